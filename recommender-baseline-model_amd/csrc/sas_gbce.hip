// SASRec head with N negatives per position: multi-negative BCE and gSASRec's generalised BCE (gfx950).
//
// The objective, on the compact valid rows rs_sas_ce_rows_fwd leaves (hl [cap][d], lab [cap], idx [cap], *count), for
// neg int64 [rows][N] read in place as neg[idx[r] * N + j] (idx == NULL: identity, and a row with lab 0 is no row):
//   valid r : pos_r != 0,  n = #valid
//   z_r0    = <f_r, E[pos_r]>                            E = item_emb.weight (tied), fp32 accumulate
//   z_rj    = <f_r, E[neg_rj]>,  j = 1..N
//   loss    = (1 / max(n, 1)) * sum_valid r [ beta * softplus(-z_r0) + sum_j softplus(z_rj) ]
//   g_r0    = s * beta * (sigmoid(z_r0) - 1),   g_rj = s * sigmoid(z_rj),   s = dloss / max(n, 1)
//   df_r    = g_r0 E[pos_r] + sum_j g_rj E[neg_rj]
//   dE[v]  += sum over (r, j = 0..N) with id_rj = v, v != 0 of  g_rj f_r
// The negatives are summed, not averaged; N = 1, beta = 1 is the reference's BCE term for term.  A negative id 0 is the
// zero row: logit exactly 0 (the table is not read), softplus(0) in the loss, no table gradient.  Nothing is masked;
// equal ids in a row are separate terms; an id outside [0, V] counts as 0.
//
// A gather kernel, not an MFMA one: every row has its own 1 + N table rows, so the bound is the gather traffic
// cap * (1 + N) * d * sizeof per pass.  One wave per row, four ids per wave pass: the 16 lanes of a lane group hold 8
// consecutive elements each of a 128-element chunk of the row (NC chunks per lane for wider rows), so one id's row is
// one 16-byte load per lane and chunk; a dot product is 8 * NC FMAs per lane and a 16-lane butterfly.
//   forward   z [cap][1 + N] into ws; each lane group adds its ids' loss terms in double in id order, the four groups
//             by two shuffles, the workgroup's four waves in wave order: part[workgroup] = {sum, valid rows, negative
//             sum}; finish_kernel adds the workgroups' partials in a fixed order.  No atomics.
//   backward  reads z; writes the weights w = g [cap][1 + N], the index keys [cap * (1 + N)] and dh = df (one fp32
//             slab): each lane group accumulates its ids' g E[id] in id order, the four groups by two shuffles.
// softplus / sigmoid use expf / log1pf (no fast intrinsics) in forms that cannot overflow.
// The table's gradient is rs_item_grad_weighted's (itemgrad.hip) over an index built on keys.
#include "common.h"
#include "../../include/recsys_hip.h"

namespace gbce {

constexpr int64_t NMAX = 1024;     // most negatives per position (rs_sas_gbce_max_n)
constexpr int DMAX = 1024;
constexpr int IDS = 4;             // ids per wave pass (one per 16-lane group)
constexpr int CW = 128;            // elements of a row chunk: 16 lanes x 8

struct Args {
  const void* hl;
  int64_t ldh;
  const int64_t* lab;
  const int32_t* idx;
  const int32_t* cnt;
  int64_t cap;
  const void* E;
  int64_t V1;
  const int64_t* neg;
  int64_t N;
  int d, vec;
  float beta;
  float* z;
  double* part;
  const float* div;
  const float* dloss;
  float* dh;
  float* w;
  int64_t* keys;
};

__device__ __forceinline__ int32_t clamp_id(int64_t v, int64_t V1) { return (v <= 0 || v >= V1) ? 0 : (int32_t)v; }

// elements k0 .. k0 + 7 of a row of width d (zeros past d)
__device__ __forceinline__ void load8(float* o, const __bf16* row, int k0, int d, bool vec) {
  if (vec && k0 + 8 <= d) {
    load_chunk<__bf16>(o, row + k0);
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = k0 + j < d ? (float)row[k0 + j] : 0.f;
}
__device__ __forceinline__ void load8(float* o, const float* row, int k0, int d, bool vec) {
  if (vec && k0 + 8 <= d) {
    load_chunk<float>(o, row + k0);
    load_chunk<float>(o + 4, row + k0 + 4);
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = k0 + j < d ? row[k0 + j] : 0.f;
}

// log(1 + exp(x)) without overflow: max(x, 0) + log1p(exp(-|x|))
__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
// 1 / (1 + exp(-x)) without overflow
__device__ __forceinline__ float sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return (x >= 0.f ? 1.f : e) / (1.f + e);
}

template <typename T, int NC>
__global__ __launch_bounds__(256) void fwd_kernel(Args a) {
  __shared__ double sl[4], sn[4];
  __shared__ int sv[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, sub = lane & 15;
  const int d = a.d;
  const bool vec = a.vec != 0;
  const int64_t count = a.cnt ? min((int64_t)*a.cnt, a.cap) : a.cap;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave, N1 = a.N + 1;
  const T* E = (const T*)a.E;
  double lsum = 0.0, nsum = 0.0;
  int valid = 0;
  if (r < count) {
    const int32_t lab = clamp_id(a.lab[r], a.V1);
    valid = lab != 0;
    float* zr = a.z + r * N1;
    if (!valid) {                                      // a row of the dense form without a positive: no row
      for (int64_t j = lane; j < N1; j += 64) zr[j] = 0.f;
    } else {
      const int64_t* negs = a.neg + (a.idx ? (int64_t)a.idx[r] : r) * a.N;
      float fr[NC][8];
#pragma unroll
      for (int c = 0; c < NC; ++c) load8(fr[c], (const T*)a.hl + r * a.ldh, c * CW + sub * 8, d, vec);
      int32_t idn = g == 0 ? lab : clamp_id(negs[g - 1 < a.N ? g - 1 : 0], a.V1);   // the first pass's id
      for (int64_t j0 = 0; j0 < N1; j0 += IDS) {
        const int64_t j = j0 + g;
        const int32_t id = j < N1 ? idn : 0;
        if (j + IDS < N1) idn = clamp_id(negs[j + IDS - 1], a.V1);    // the next pass's, ahead of this pass's rows
        float acc = 0.f;
        if (id) {
          const T* row = E + (int64_t)id * d;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            if (c * CW < d) {
              float e[8];
              load8(e, row, c * CW + sub * 8, d, vec);
#pragma unroll
              for (int k = 0; k < 8; ++k) acc = __builtin_fmaf(fr[c][k], e[k], acc);
            }
          }
        }
        acc = group16_sum(acc);                        // every lane of the wave takes part
        const float zv = id ? acc : 0.f;
        if (j < N1) {
          if (sub == 0) zr[j] = zv;
          if (j == 0) {
            lsum += (double)(a.beta * softplus(-zv));
          } else {
            const double t = (double)softplus(zv);
            lsum += t;
            nsum += t;
          }
        }
      }
      // the four lane groups' sums in a fixed, symmetric order: every lane ends with the same bits
      lsum += __shfl_xor(lsum, 16, 64);
      lsum += __shfl_xor(lsum, 32, 64);
      nsum += __shfl_xor(nsum, 16, 64);
      nsum += __shfl_xor(nsum, 32, 64);
    }
  }
  if (lane == 0) {
    sl[wave] = lsum;
    sn[wave] = nsum;
    sv[wave] = valid;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.part[3 * (int64_t)blockIdx.x + 0] = ((sl[0] + sl[1]) + sl[2]) + sl[3];
    a.part[3 * (int64_t)blockIdx.x + 1] = (double)(sv[0] + sv[1] + sv[2] + sv[3]);
    a.part[3 * (int64_t)blockIdx.x + 2] = ((sn[0] + sn[1]) + sn[2]) + sn[3];
  }
}

// out = {loss sum, valid rows, sum / *div, negative-term sum}: one workgroup, a fixed order
__global__ __launch_bounds__(256) void finish_kernel(const double* __restrict__ part, int64_t nb, const float* div,
                                                     float* __restrict__ out) {
  __shared__ double red[3][256];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < nb; b += 256) {
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q] += part[3 * b + q];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) red[q][threadIdx.x] = acc[q];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
#pragma unroll
      for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)red[0][0];
    out[1] = (float)red[1][0];
    out[2] = (float)(red[0][0] / (double)*div);
    out[3] = (float)red[2][0];
  }
}

template <typename T, int NC>
__global__ __launch_bounds__(256) void bwd_kernel(Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, sub = lane & 15;
  const int d = a.d;
  const bool vec = a.vec != 0;
  const int64_t count = a.cnt ? min((int64_t)*a.cnt, a.cap) : a.cap;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave, N1 = a.N + 1;
  if (r >= a.cap) return;
  int64_t* kr = a.keys + r * N1;
  if (r >= count) {                                    // past the count: key 0 = no entry; nothing else is written
    for (int64_t j = lane; j < N1; j += 64) kr[j] = 0;
    return;
  }
  const T* E = (const T*)a.E;
  float* wr = a.w + r * N1;
  float* dhr = a.dh + r * d;
  const int32_t lab = clamp_id(a.lab[r], a.V1);
  if (!lab) {                                          // a row of the dense form without a positive: zero gradients
    for (int64_t j = lane; j < N1; j += 64) {
      kr[j] = 0;
      wr[j] = 0.f;
    }
    for (int k = lane; k < d; k += 64) dhr[k] = 0.f;
    return;
  }
  const float s = (a.dloss ? *a.dloss : 1.f) / *a.div;
  const int64_t* negs = a.neg + (a.idx ? (int64_t)a.idx[r] : r) * a.N;
  const float* zr = a.z + r * N1;
  float acc[NC][8];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[c][k] = 0.f;
  int32_t idn = g == 0 ? lab : clamp_id(negs[g - 1 < a.N ? g - 1 : 0], a.V1);
  for (int64_t j0 = 0; j0 < N1; j0 += IDS) {
    const int64_t j = j0 + g;
    const int32_t id = j < N1 ? idn : 0;
    if (j + IDS < N1) idn = clamp_id(negs[j + IDS - 1], a.V1);
    if (j >= N1) continue;
    const float zv = zr[j];
    // sigmoid(z) - 1 = -sigmoid(-z): no cancellation at large z
    const float gv = j == 0 ? -(s * a.beta) * sigmoid(-zv) : s * sigmoid(zv);
    if (sub == 0) {
      wr[j] = gv;
      kr[j] = id;
    }
    if (id) {
      const T* row = E + (int64_t)id * d;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c * CW < d) {
          float e[8];
          load8(e, row, c * CW + sub * 8, d, vec);
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[c][k] = __builtin_fmaf(gv, e[k], acc[c][k]);
        }
      }
    }
  }
  // the four lane groups' sums: ((g0 + g1) + (g2 + g3)) in every lane
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float v = acc[c][k];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      acc[c][k] = v;
    }
  if (g == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int k0 = c * CW + sub * 8;
      if (vec && k0 + 8 <= d) {
        store_chunk<float>(dhr + k0, acc[c]);
        store_chunk<float>(dhr + k0 + 4, acc[c] + 4);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k0 + k < d) dhr[k0 + k] = acc[c][k];
      }
    }
  }
}

static bool supported(int dtype, int64_t d, int64_t N) {
  if (dtype != RS_DTYPE_F32 && dtype != RS_DTYPE_BF16) return false;
  if (d < 1 || d > DMAX || (dtype == RS_DTYPE_BF16 && d % 8)) return false;
  return N >= 1 && N <= NMAX;
}

static bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// the workspace: z fp32 [cap][1 + N] | part (double) [workgroups][3]
static int64_t part_offset(int64_t cap, int64_t N) { return (4 * cap * (N + 1) + 15) / 16 * 16; }

template <typename T, bool BWD>
static void launch_t(int64_t d, int64_t cap, hipStream_t s, const Args& a) {
  const dim3 grid((unsigned)cdiv(cap, (int64_t)4)), block(256);
  if (d <= CW) {
    if (BWD) hipLaunchKernelGGL((bwd_kernel<T, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((fwd_kernel<T, 1>), grid, block, 0, s, a);
  } else if (d <= 2 * CW) {
    if (BWD) hipLaunchKernelGGL((bwd_kernel<T, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((fwd_kernel<T, 2>), grid, block, 0, s, a);
  } else if (d <= 4 * CW) {
    if (BWD) hipLaunchKernelGGL((bwd_kernel<T, 4>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((fwd_kernel<T, 4>), grid, block, 0, s, a);
  } else {
    if (BWD) hipLaunchKernelGGL((bwd_kernel<T, 8>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((fwd_kernel<T, 8>), grid, block, 0, s, a);
  }
}

static int check(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab, const void* E,
                 int64_t V1, const int64_t* neg, int64_t N, const float* divisor, const void* ws) {
  if (!supported(dtype, d, N)) return RS_ERR_UNSUPPORTED;
  if (cap <= 0 || cap * (N + 1) >= ((int64_t)1 << 31)) return RS_ERR_UNSUPPORTED;
  if (V1 < 1 || V1 >= ((int64_t)1 << 31) || !hl || !lab || !E || !neg || !divisor || !ws || ldh < d || !al16(ws))
    return RS_ERR_ARG;
  return 0;
}

static Args make_args(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                      const int32_t* idx, const int32_t* count, const void* E, int64_t V1, const int64_t* neg,
                      int64_t N, float beta, const float* divisor, void* ws) {
  const int64_t sz = dtype == RS_DTYPE_BF16 ? 2 : 4;
  Args a = {};
  a.hl = hl; a.ldh = ldh; a.lab = lab; a.idx = idx; a.cnt = count; a.cap = cap; a.E = E; a.V1 = V1; a.neg = neg;
  a.N = N; a.d = (int)d; a.beta = beta; a.div = divisor;
  // 16-byte chunks of 8 (bf16) or 4 + 4 (fp32) elements: every row base and pitch a multiple of 16 bytes
  a.vec = al16(hl) && al16(E) && (ldh * sz) % 16 == 0 && (d * sz) % 16 == 0;
  a.z = (float*)ws;
  a.part = (double*)((char*)ws + part_offset(cap, N));
  return a;
}

}  // namespace gbce

extern "C" {

int64_t rs_sas_gbce_max_n(void) { return gbce::NMAX; }

int64_t rs_sas_gbce_ws_bytes(int64_t cap, int64_t N, int64_t d) {
  if (cap <= 0 || N <= 0 || d <= 0 || N > gbce::NMAX || cap * (N + 1) >= ((int64_t)1 << 31)) return -1;
  return gbce::part_offset(cap, N) + 8 * 3 * cdiv(cap, (int64_t)4);
}

int rs_sas_gbce_fwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                    const int32_t* idx, const int32_t* count, const void* E, int64_t V1, const int64_t* neg, int64_t N,
                    float beta, const float* divisor, void* ws, float* out, void* stream) {
  if (int e = gbce::check(dtype, cap, d, hl, ldh, lab, E, V1, neg, N, divisor, ws)) return e;
  if (!out) return RS_ERR_ARG;
  const gbce::Args a = gbce::make_args(dtype, cap, d, hl, ldh, lab, idx, count, E, V1, neg, N, beta, divisor, ws);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RS_DTYPE_BF16) gbce::launch_t<__bf16, false>(d, cap, s, a);
  else gbce::launch_t<float, false>(d, cap, s, a);
  hipLaunchKernelGGL(gbce::finish_kernel, dim3(1), dim3(256), 0, s, a.part, cdiv(cap, (int64_t)4), divisor, out);
  return (int)hipGetLastError();
}

int rs_sas_gbce_bwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                    const int32_t* idx, const int32_t* count, const void* E, int64_t V1, const int64_t* neg, int64_t N,
                    float beta, const float* divisor, const float* dloss, void* ws, float* dh, float* w, int64_t* keys,
                    void* stream) {
  if (int e = gbce::check(dtype, cap, d, hl, ldh, lab, E, V1, neg, N, divisor, ws)) return e;
  if (!dh || !w || !keys) return RS_ERR_ARG;
  gbce::Args a = gbce::make_args(dtype, cap, d, hl, ldh, lab, idx, count, E, V1, neg, N, beta, divisor, ws);
  a.vec = a.vec && gbce::al16(dh) && (d * 4) % 16 == 0;
  a.dloss = dloss; a.dh = dh; a.w = w; a.keys = keys;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RS_DTYPE_BF16) gbce::launch_t<__bf16, true>(d, cap, s, a);
  else gbce::launch_t<float, true>(d, cap, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
