// Sparse (touched-rows-only) Adam for the embedding / output tables (gfx950): the optimizer of a sampled-loss step
// in O(touched rows) instead of O(table rows).
//
//   rs_unique_rows : up to three int64 key arrays -> the ascending list of the distinct keys in [1, table_rows) as
//                    int32 rows[cap] and a device count.  Flag / count / scan / emit over the table's rows in ints
//                    (sparse_rows.hip's scheme with the inversion done by the last launch): five launches, no host
//                    synchronisation, no atomics -- the list is a pure function of the key SET.
//                    Workspace: 4 * (table_rows + 2 * ceil(table_rows / 2048)) bytes (rs_unique_rows_ws_bytes): one
//                    int32 flag per table row and two int32 per scan block; never a multiple of the row width.
//   rs_adam_rows   : the dense sweep's per-element update (adam_math.h, the step's scalars from state[1..3]) on the
//                    listed rows only; every other row of p / m / v / p_bf16 / g is neither read nor written.
//
// rs_adam_rows is a gather / scatter of a few ten thousand rows of 4 B .. 4 KB and is latency-bound: the listed rows
// are flattened into one array of 16-byte chunks (row = chunk / chunks-per-row by a 32-bit division), so consecutive
// lanes take consecutive chunks of a row and run on into the next listed row -- a wave covers 64 / (d / 4) whole rows
// per pass at d <= 256 and loops over a longer one -- and every thread issues the p / g / m / v loads of AR_U chunks
// (16 loads, up to AR_U different rows) before the first update.  Plain loads and stores: the rows a Zipf batch touches
// are the popular ones, which the next step reads again from the caches.
#include "adam_math.h"
#include "common.h"
#include "../../include/recsys_hip.h"

namespace ar {

constexpr int NT = 256;
constexpr int PER = 8;                // flags per thread
constexpr int CH = NT * PER;          // flags per scan block
constexpr int AR_U = 4;               // chunks (elements on the scalar path) in flight per thread

__global__ __launch_bounds__(NT) void zero_kernel(int32_t* __restrict__ flags, int64_t rows) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < rows; i += (int64_t)gridDim.x * NT) flags[i] = 0;
}

struct Keys { const int64_t* k[3]; int64_t n[3]; };

__global__ __launch_bounds__(NT) void mark_kernel(Keys ks, int64_t total, int64_t rows, int32_t* __restrict__ flags) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    int64_t j = i;
    int s = 0;
    while (j >= ks.n[s]) j -= ks.n[s++];      // total = n0 + n1 + n2: s stays below 3
    const int64_t v = ks.k[s][j];
    if (v >= 1 && v < rows) flags[v] = 1;     // benign race: every writer stores 1
  }
}

// block-wide exclusive scan of one value per thread; returns the exclusive prefix, *total = block sum
__device__ __forceinline__ int32_t block_scan(int32_t x, int32_t* sh, int32_t* total) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int32_t v = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t y = __shfl_up(v, o, 64);
    if (lane >= o) v += y;
  }
  if (lane == 63) sh[w] = v;
  __syncthreads();
  int32_t wofs = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    if (k < w) wofs += sh[k];
    tot += sh[k];
  }
  __syncthreads();
  *total = tot;
  return wofs + v - x;
}

__global__ __launch_bounds__(NT) void count_kernel(const int32_t* __restrict__ flags, int64_t rows,
                                                   int32_t* __restrict__ bsum) {
  __shared__ int32_t sh[NT / 64];
  const int64_t base = (int64_t)blockIdx.x * CH + threadIdx.x * PER;
  int32_t c = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) c += (base + k < rows) ? flags[base + k] : 0;
  int32_t tot;
  block_scan(c, sh, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// exclusive scan of the block counts (one workgroup, any number of blocks) -> bofs, *count
__global__ __launch_bounds__(NT) void scan_blocks_kernel(const int32_t* __restrict__ bsum, int64_t nb,
                                                         int32_t* __restrict__ bofs, int32_t* __restrict__ count) {
  __shared__ int32_t sh[NT / 64];
  int32_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += NT) {
    const int64_t b = b0 + threadIdx.x;
    const int32_t x = b < nb ? bsum[b] : 0;
    int32_t tot;
    const int32_t ex = block_scan(x, sh, &tot);
    if (b < nb) bofs[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *count = carry;
}

// the inversion: list[rank of v among the flagged rows] = v.  A flagged row's rank is below the number of in-range
// keys, so below cap (host-checked cap >= n0 + n1 + n2); the bound is tested all the same.
__global__ __launch_bounds__(NT) void emit_kernel(const int32_t* __restrict__ flags, int64_t rows,
                                                  const int32_t* __restrict__ bofs, int32_t* __restrict__ list,
                                                  int64_t cap) {
  __shared__ int32_t sh[NT / 64];
  const int64_t base = (int64_t)blockIdx.x * CH + threadIdx.x * PER;
  int32_t f[PER], c = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    f[k] = (base + k < rows) ? flags[base + k] : 0;
    c += f[k];
  }
  int32_t tot;
  int32_t pos = bofs[blockIdx.x] + block_scan(c, sh, &tot);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (f[k] && pos < cap) list[pos] = (int32_t)(base + k);
    pos += f[k];
  }
}

static unsigned grid_for(int64_t work, int64_t per_block) {
  const int64_t g = cdiv(work, per_block);
  return (unsigned)(g < 2048 ? (g > 0 ? g : 1) : 2048);
}

// VEC: W = 4 elements per item (one float4 of a row), cpr = d / 4 items per row; else W = 1, cpr = d.
template <bool BF16OUT, bool VEC>
__global__ __launch_bounds__(NT) void adam_rows_kernel(uint32_t cpr, int64_t d, int64_t table_rows,
                                                       const int32_t* __restrict__ list,
                                                       const int32_t* __restrict__ count, int64_t cap,
                                                       float* __restrict__ p, float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       __bf16* __restrict__ pb, const double* __restrict__ state,
                                                       const double* __restrict__ hyper, int zero_grad) {
  constexpr int W = VEC ? 4 : 1;
  const AdamElem h = adam_elem(hyper);
  const float step_size = (float)state[1], bc2s = (float)state[2], gs = (float)state[3];
  int64_t n = *count;
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const uint32_t total = (uint32_t)n * cpr;         // host-checked: cap * cpr < 2^31
  const uint32_t stride = gridDim.x * NT;
  for (uint32_t q0 = blockIdx.x * NT + threadIdx.x; q0 < total; q0 += AR_U * stride) {
    int64_t e[AR_U];
    bool ok[AR_U];
    float P[AR_U][W], G[AR_U][W], M[AR_U][W], V[AR_U][W];
#pragma unroll
    for (int u = 0; u < AR_U; ++u) {
      const uint32_t q = q0 + u * stride;
      ok[u] = q < total && q >= q0;                  // q >= q0: no wrap past 2^32
      int64_t r = -1;
      uint32_t c = 0;
      if (ok[u]) {
        const uint32_t i = q / cpr;
        c = q - i * cpr;
        r = list[i];
      }
      ok[u] = ok[u] && r >= 0 && r < table_rows;     // an id outside the table is skipped, never dereferenced
      e[u] = r * d + (int64_t)c * W;
    }
    // every load of the group before the first update: up to AR_U rows' round trips overlap
#pragma unroll
    for (int u = 0; u < AR_U; ++u) {
#pragma unroll
      for (int j = 0; j < W; ++j) P[u][j] = G[u][j] = M[u][j] = V[u][j] = 0.f;
      if (ok[u]) {
        if (VEC) {
          const float4 a = *reinterpret_cast<const float4*>(p + e[u]);
          const float4 b = *reinterpret_cast<const float4*>(g + e[u]);
          const float4 c4 = *reinterpret_cast<const float4*>(m + e[u]);
          const float4 d4 = *reinterpret_cast<const float4*>(v + e[u]);
          P[u][0] = a.x; P[u][1 % W] = a.y; P[u][2 % W] = a.z; P[u][3 % W] = a.w;
          G[u][0] = b.x; G[u][1 % W] = b.y; G[u][2 % W] = b.z; G[u][3 % W] = b.w;
          M[u][0] = c4.x; M[u][1 % W] = c4.y; M[u][2 % W] = c4.z; M[u][3 % W] = c4.w;
          V[u][0] = d4.x; V[u][1 % W] = d4.y; V[u][2 % W] = d4.z; V[u][3 % W] = d4.w;
        } else {
          P[u][0] = p[e[u]]; G[u][0] = g[e[u]]; M[u][0] = m[e[u]]; V[u][0] = v[e[u]];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < AR_U; ++u) {
      if (!ok[u]) continue;
      bool gnz = false;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        gnz = gnz || __float_as_uint(G[u][j]) != 0u;
        adam_elem_update(P[u][j], G[u][j], M[u][j], V[u][j], h, step_size, bc2s, gs);
      }
      if (VEC) {
        *reinterpret_cast<float4*>(p + e[u]) = make_float4(P[u][0], P[u][1 % W], P[u][2 % W], P[u][3 % W]);
        *reinterpret_cast<float4*>(m + e[u]) = make_float4(M[u][0], M[u][1 % W], M[u][2 % W], M[u][3 % W]);
        *reinterpret_cast<float4*>(v + e[u]) = make_float4(V[u][0], V[u][1 % W], V[u][2 % W], V[u][3 % W]);
        if (zero_grad && gnz) *reinterpret_cast<float4*>(g + e[u]) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (BF16OUT) {
          bf16x4 o;
          o[0] = (__bf16)P[u][0]; o[1] = (__bf16)P[u][1 % W]; o[2] = (__bf16)P[u][2 % W]; o[3] = (__bf16)P[u][3 % W];
          *reinterpret_cast<bf16x4*>(pb + e[u]) = o;
        }
      } else {
        p[e[u]] = P[u][0]; m[e[u]] = M[u][0]; v[e[u]] = V[u][0];
        if (zero_grad && gnz) g[e[u]] = 0.f;
        if (BF16OUT) pb[e[u]] = (__bf16)P[u][0];
      }
    }
  }
}

}  // namespace ar

extern "C" {

int64_t rs_unique_rows_ws_bytes(int64_t table_rows) {
  if (table_rows <= 0) return -1;
  return 4 * (table_rows + 2 * cdiv(table_rows, (int64_t)ar::CH));
}

int rs_unique_rows(const int64_t* keys0, int64_t n0, const int64_t* keys1, int64_t n1, const int64_t* keys2,
                   int64_t n2, int64_t table_rows, int32_t* rows, int32_t* count, int64_t cap, void* ws,
                   int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0 || n2 < 0 || table_rows <= 0 || table_rows >= (1ll << 31) || !rows || !count || !ws)
    return RS_ERR_ARG;
  if ((n0 && !keys0) || (n1 && !keys1) || (n2 && !keys2)) return RS_ERR_ARG;
  const int64_t total = n0 + n1 + n2;
  if (cap < total || cap < 1 || ws_bytes < rs_unique_rows_ws_bytes(table_rows) || (uintptr_t)ws % 4) return RS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nb = cdiv(table_rows, (int64_t)ar::CH);
  int32_t* flags = (int32_t*)ws;
  int32_t* bsum = flags + table_rows;
  int32_t* bofs = bsum + nb;
  ar::Keys ks{{keys0, keys1, keys2}, {n0, n1, n2}};
  hipLaunchKernelGGL(ar::zero_kernel, dim3(ar::grid_for(table_rows, ar::NT * 4)), dim3(ar::NT), 0, s, flags,
                     table_rows);
  if (total > 0)
    hipLaunchKernelGGL(ar::mark_kernel, dim3(ar::grid_for(total, ar::NT * 4)), dim3(ar::NT), 0, s, ks, total,
                       table_rows, flags);
  hipLaunchKernelGGL(ar::count_kernel, dim3((unsigned)nb), dim3(ar::NT), 0, s, flags, table_rows, bsum);
  hipLaunchKernelGGL(ar::scan_blocks_kernel, dim3(1), dim3(ar::NT), 0, s, bsum, nb, bofs, count);
  hipLaunchKernelGGL(ar::emit_kernel, dim3((unsigned)nb), dim3(ar::NT), 0, s, flags, table_rows, bofs, rows, cap);
  return (int)hipGetLastError();
}

int rs_adam_rows(int64_t d, int64_t table_rows, const int32_t* rows, const int32_t* count, int64_t cap, float* p,
                 float* g, float* m, float* v, void* p_bf16, const double* state, const double* hyper, int zero_grad,
                 int max_wg, void* stream) {
  if (d <= 0 || table_rows <= 0 || cap <= 0 || max_wg <= 0 || !rows || !count || !p || !g || !m || !v || !state ||
      !hyper)
    return RS_ERR_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 4 || (uintptr_t)p_bf16 % 2) return RS_ERR_ARG;
  const bool vec = d % 4 == 0 && ((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0 &&
                   (uintptr_t)p_bf16 % 8 == 0;
  const int64_t cpr = vec ? d / 4 : d;
  if (cpr >= (1ll << 31) / cap) return RS_ERR_ARG;          // the flattened item index is 32 bits
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(cdiv(cap * cpr, (int64_t)ar::NT * ar::AR_U), max_wg));
  hipStream_t s = (hipStream_t)stream;
#define AR_LAUNCH(BO, VE)                                                                                         \
  hipLaunchKernelGGL((ar::adam_rows_kernel<BO, VE>), dim3((unsigned)blocks), dim3(ar::NT), 0, s, (uint32_t)cpr, d, \
                     table_rows, rows, count, cap, p, g, m, v, (__bf16*)p_bf16, state, hyper, zero_grad)
  if (p_bf16) {
    if (vec) AR_LAUNCH(true, true);
    else AR_LAUNCH(true, false);
  } else {
    if (vec) AR_LAUNCH(false, true);
    else AR_LAUNCH(false, false);
  }
#undef AR_LAUNCH
  return (int)hipGetLastError();
}

}  // extern "C"
