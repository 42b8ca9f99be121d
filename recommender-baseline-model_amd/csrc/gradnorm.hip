// Global gradient norm and clip coefficient of a training step (gfx950): torch.nn.utils.clip_grad_norm_(params, c)
// for the fused step, where nothing can run between the backward and the optimizer.  Three kernels, all in double:
//
//   rs_gradnorm_dense   sum of squares over one or more ranges [lo, hi) of the flat fp32 gradient -> double partials
//   rs_gradnorm_rows    the same over the rows rows[0 .. *count) of a table [R][d] (rs_unique_rows' list) and over no
//                       other row: a sparse-table step's norm costs O(touched rows), as its optimizer does
//   rs_gradnorm_finish  one workgroup: the sum of every partial, norm = sqrt(sum) / div, torch's coefficient
//                       min(1, max_norm / (norm + 1e-6)) and the divisor the optimizer kernels take in place of div
//
// The square of an fp32 is exact in fp64 (24 + 24 <= 53 bits), so the only roundings are the additions'.
//
// Fixed arithmetic, whatever the grid.  A range (a list) is summed by a VIRTUAL grid whose size follows from its
// length alone (dense_vb / rows_vb below); virtual workgroup v owns partial slot v.  Thread t of v takes the items
// (one float4, or one element on the scalar row path) v * 256 + t + k * (virtual workgroups * 256), k = 0, 1, ..., in
// that order, into four accumulators (one per float4 component; the range's n % 4 tail elements go to thread t <
// n % 4 of v = 0, into component 0, last), then s = (s0 + s1) + (s2 + s3), a 64-lane xor butterfly (offsets 32 .. 1)
// and ((w0 + w1) + w2) + w3 over the four waves.  The launch's real workgroups (at most max_wg) walk the virtual ones
// grid-stride, so max_wg moves work between CUs and never changes a bit.  Every virtual workgroup stores its slot
// every launch -- a zero when the list is short -- so a replayed graph never reads a stale partial.
//
// No atomics and no "last workgroup reduces" pass (a per-workgroup __threadfence() made an optimizer launch 30 us on
// gfx950, misc.hip): partial launches, then the finish launch, as penalty.hip's sumsq_kernel -> norm_kernel.
#include "common.h"
#include "../../include/recsys_hip.h"

namespace gn {

constexpr int NT = 256;
constexpr int U = 4;               // items in flight per thread
constexpr int DENSE_VB = 2048;     // virtual workgroups of one dense range at most (8 per CU: one resident wave)
constexpr int ROWS_VB = 1024;      // ... of one row list
constexpr int MAX_RANGES = 8;

__host__ __device__ static inline int64_t dense_vb(int64_t n) {
  const int64_t v = cdiv(n / 4, (int64_t)NT * U);
  return v < 1 ? 1 : (v > DENSE_VB ? DENSE_VB : v);
}
// from cap and d alone (not from the access width), so the slot count is known before the pointers are
static inline int64_t rows_vb(int64_t d, int64_t cap) {
  const int64_t v = cdiv(cap * d, (int64_t)4 * NT * U);
  return v < 1 ? 1 : (v > ROWS_VB ? ROWS_VB : v);
}

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) red[w] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

__device__ __forceinline__ void acc4(double* s, const float4 x) {
  const double a = x.x, b = x.y, c = x.z, d = x.w;
  s[0] = __builtin_fma(a, a, s[0]);      // a * a is exact: one rounding, the addition's
  s[1] = __builtin_fma(b, b, s[1]);
  s[2] = __builtin_fma(c, c, s[2]);
  s[3] = __builtin_fma(d, d, s[3]);
}

struct Ranges {
  int64_t lo[MAX_RANGES], n[MAX_RANGES];
  int64_t first[MAX_RANGES + 1];     // first virtual workgroup (= partial slot) of each range; [nr] = their number
  int nr;
};

__global__ __launch_bounds__(NT) void dense_kernel(const float* __restrict__ g, Ranges rg,
                                                   double* __restrict__ partials) {
  __shared__ double red[NT / 64];
  const int64_t total = rg.first[rg.nr];
  for (int64_t vb = blockIdx.x; vb < total; vb += gridDim.x) {
    int r = 0;
    while (r + 1 < rg.nr && vb >= rg.first[r + 1]) ++r;
    const int64_t v = vb - rg.first[r], nv = rg.first[r + 1] - rg.first[r];
    const float* __restrict__ x = g + rg.lo[r];
    const int64_t n = rg.n[r], n4 = n / 4, stride = nv * NT;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t i = v * NT + threadIdx.x;
    for (; i + (U - 1) * stride < n4; i += U * stride) {
      float4 q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = reinterpret_cast<const float4*>(x)[i + u * stride];
#pragma unroll
      for (int u = 0; u < U; ++u) acc4(s, q[u]);
    }
    for (; i < n4; i += stride) acc4(s, reinterpret_cast<const float4*>(x)[i]);
    if (v == 0 && (int64_t)threadIdx.x < (n & 3)) {
      const double a = x[n4 * 4 + threadIdx.x];
      s[0] = __builtin_fma(a, a, s[0]);
    }
    const double t = block_sum((s[0] + s[1]) + (s[2] + s[3]), red);
    if (threadIdx.x == 0) partials[vb] = t;
  }
}

// VEC: an item is one float4 of a listed row (cpr = d / 4 items per row), else one element (cpr = d); the listed rows
// flattened into one item array, rs_adam_rows' access shape
template <bool VEC>
__global__ __launch_bounds__(NT) void rows_kernel(uint32_t cpr, int64_t d, int64_t table_rows,
                                                  const int32_t* __restrict__ list,
                                                  const int32_t* __restrict__ count, int64_t cap,
                                                  const float* __restrict__ g, int nv,
                                                  double* __restrict__ partials) {
  __shared__ double red[NT / 64];
  int64_t n = *count;
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const uint32_t total = (uint32_t)n * cpr;          // host-checked: cap * d < 2^31
  const uint32_t stride = (uint32_t)nv * NT;         // <= 2^18: q0 + U * stride stays below 2^32
  for (int v = blockIdx.x; v < nv; v += gridDim.x) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t q0 = (uint32_t)v * NT + threadIdx.x; q0 < total; q0 += U * stride) {
      float4 x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t q = q0 + u * stride;
        x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < total) {
          const uint32_t i = q / cpr, c = q - i * cpr;
          const int64_t r = list[i];
          if (r >= 0 && r < table_rows) {            // an id outside the table is skipped, never dereferenced
            if (VEC) x[u] = *reinterpret_cast<const float4*>(g + r * d + (int64_t)c * 4);
            else x[u].x = g[r * d + c];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc4(s, x[u]);
    }
    const double t = block_sum((s[0] + s[1]) + (s[2] + s[3]), red);
    if (threadIdx.x == 0) partials[v] = t;
  }
}

// thread t: partials t, t + 256, ... in index order; then block_sum.  rec = {norm, coef, effective divisor}
__global__ __launch_bounds__(NT) void finish_kernel(const double* __restrict__ partials, int64_t nparts,
                                                    const float* __restrict__ div,
                                                    const double* __restrict__ max_norm, float* __restrict__ rec) {
  __shared__ double red[NT / 64];
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < nparts; k += NT) s += partials[k];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const float dv = div ? div[0] : 1.f;
    const double nrm = __dsqrt_rn(s) / (double)dv;
    const double e = nrm + 1e-6, mx = max_norm[0];
    const float coef = (float)(mx / e);
    const bool clip = !(coef >= 1.f);                // a NaN coefficient is applied, as torch's clamp(max=1) keeps it
    rec[0] = (float)nrm;
    rec[1] = clip ? coef : 1.f;
    rec[2] = clip ? (float)((double)dv * e / mx) : dv;
  }
}

}  // namespace gn

extern "C" {

int64_t rs_gradnorm_dense_parts(int64_t n) { return n <= 0 ? -1 : gn::dense_vb(n); }

int64_t rs_gradnorm_rows_parts(int64_t d, int64_t cap) {
  if (d < 1 || cap < 1 || d >= (1ll << 31) / cap) return -1;
  return gn::rows_vb(d, cap);
}

int rs_gradnorm_dense(const float* g, const int64_t* ranges, int nranges, int max_wg, double* partials,
                      void* stream) {
  if (!g || (uintptr_t)g % 16 || !ranges || nranges < 1 || nranges > gn::MAX_RANGES || max_wg < 1 || !partials ||
      (uintptr_t)partials % 8)
    return RS_ERR_ARG;
  gn::Ranges rg;
  rg.nr = nranges;
  rg.first[0] = 0;
  for (int r = 0; r < nranges; ++r) {
    const int64_t lo = ranges[2 * r], hi = ranges[2 * r + 1];
    if (lo < 0 || lo % 4 || hi <= lo) return RS_ERR_ARG;      // n <= 0, or a range start off the 16-byte grid
    rg.lo[r] = lo;
    rg.n[r] = hi - lo;
    rg.first[r + 1] = rg.first[r] + gn::dense_vb(hi - lo);
  }
  for (int r = nranges; r < gn::MAX_RANGES; ++r) rg.lo[r] = rg.n[r] = 0, rg.first[r + 1] = rg.first[nranges];
  const int64_t blocks = std::min<int64_t>(rg.first[nranges], max_wg);
  hipLaunchKernelGGL(gn::dense_kernel, dim3((unsigned)blocks), dim3(gn::NT), 0, (hipStream_t)stream, g, rg, partials);
  return (int)hipGetLastError();
}

int rs_gradnorm_rows(const float* g, int64_t d, int64_t table_rows, const int32_t* rows, const int32_t* count,
                     int64_t cap, int max_wg, double* partials, void* stream) {
  if (!g || (uintptr_t)g % 4 || d < 1 || table_rows < 1 || cap < 1 || max_wg < 1 || !rows || !count || !partials ||
      (uintptr_t)partials % 8)
    return RS_ERR_ARG;
  if (d >= (1ll << 31) / cap) return RS_ERR_ARG;              // the flattened item index is 32 bits
  const bool vec = d % 4 == 0 && (uintptr_t)g % 16 == 0;
  const int nv = (int)gn::rows_vb(d, cap);
  const int blocks = std::min(nv, max_wg);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(gn::rows_kernel<true>, dim3((unsigned)blocks), dim3(gn::NT), 0, s, (uint32_t)(d / 4), d,
                       table_rows, rows, count, cap, g, nv, partials);
  else
    hipLaunchKernelGGL(gn::rows_kernel<false>, dim3((unsigned)blocks), dim3(gn::NT), 0, s, (uint32_t)d, d, table_rows,
                       rows, count, cap, g, nv, partials);
  return (int)hipGetLastError();
}

int rs_gradnorm_finish(const double* partials, int64_t nparts, const float* div, const double* max_norm, float* record,
                       void* stream) {
  if (!partials || (uintptr_t)partials % 8 || nparts < 1 || nparts > (1ll << 24) || !max_norm ||
      (uintptr_t)max_norm % 8 || !record || (uintptr_t)record % 4 || (uintptr_t)div % 4)
    return RS_ERR_ARG;
  hipLaunchKernelGGL(gn::finish_kernel, dim3(1), dim3(gn::NT), 0, (hipStream_t)stream, partials, nparts, div, max_norm,
                     record);
  return (int)hipGetLastError();
}

}  // extern "C"
