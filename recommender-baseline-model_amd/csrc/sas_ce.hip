// Row kernels of the SASRec tied full-catalogue cross-entropy head (gfx950; bf16, d in {64, 128}).
//
// The objective: f = LN_last(x_L); logits = f E^T over the whole item table E (tied: E = item_emb, class 0 = the
// zero padding row); CrossEntropy(ignore_index=0) against the next item `pos`.  Rows with pos == 0 carry neither
// loss nor gradient (left-padded sequences: about 5 of 6 rows at the Beauty lengths), so the vocabulary kernels
// (vocab_head.hip) run on the compacted valid rows only.  These two kernels are the row-local work on each side of
// them, one launch each:
//   rs_sas_ce_rows_fwd   rs_compact_rows + rs_layernorm_fwd (variant 0) + rs_gather_rows: the last LayerNorm runs
//                        on the valid rows only and lands in the compact buffer directly
//   rs_sas_ce_rows_bwd   rs_splitk_scatter_rows + rs_layernorm_bwd: the split-K slabs of dh = dlogits E summed in
//                        split order, the LayerNorm backward, dx scattered to all M rows (zeros at invalid rows),
//                        the affine partials left per workgroup for the grouped reduction (ops.ln_partial_segments)
// Same arithmetic, in the same order, as the launches they replace (layernorm.hip's vectorised kernels, rows.hip),
// no atomics: results are reproducible run to run.
#include "common.h"
#include "../../include/recsys_hip.h"

#define SCE_BWD_BLOCKS 512   // affine-partial sets at most (as LN_BWD_BLOCKS)
#define SCE_BWD_ROWS 16      // rows per partial set and sweep at least (d = 128: 16 lanes per row, 4 waves)

template <int LPR>
__device__ __forceinline__ float sce_group_sum(float v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One 1024-row block per workgroup.  Placement exactly as compact_kernel (rows.hip): the valid rows before the
// block counted by strided loads and one reduction, the block's own rows placed by wave ballots.  The block's
// valid rows are then listed in LDS and its 16 waves normalise them, LPR lanes (one 16-byte chunk each) per row.
template <int LPR>
__global__ __launch_bounds__(1024) void sas_ce_rows_fwd_kernel(const int64_t* __restrict__ labels, int64_t n,
                                                               int64_t cap, const __bf16* __restrict__ X, int64_t ldx,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps,
                                                               int32_t* __restrict__ idx, int32_t* __restrict__ rank,
                                                               int32_t* __restrict__ count,
                                                               float* __restrict__ divisor, __bf16* __restrict__ HL,
                                                               int64_t ldh, int64_t* __restrict__ lab_out,
                                                               float* __restrict__ mean_out,
                                                               float* __restrict__ rstd_out) {
  // contraction spelled out as in ln_fwd_v_kernel: the same bits as rs_layernorm_fwd on the same row
#pragma clang fp contract(off)
  constexpr int V = 8, RPW = 64 / LPR, d = LPR * V;
  __shared__ int32_t wb[16], wo[16], wpre[18];
  __shared__ int32_t rows[1024];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * 1024, r = base + tid;
  const bool lab = r < n && labels[r] != 0;
  int32_t c = 0;
  for (int64_t q = tid; q < base; q += 1024) c += labels[q] != 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  const uint64_t bal = __ballot(lab);
  if (lane == 0) {
    wb[w] = c;
    wo[w] = (int32_t)__popcll(bal);
  }
  __syncthreads();
  if (tid == 0) {
    int32_t before = 0, own = 0;
    for (int k = 0; k < 16; ++k) {
      wpre[k] = own;
      before += wb[k];
      own += wo[k];
    }
    wpre[16] = before;
    wpre[17] = own;
  }
  __syncthreads();
  const int32_t before = wpre[16], own = wpre[17];
  const int32_t li = wpre[w] + (int32_t)__popcll(bal & ((1ull << lane) - 1ull));   // place among the block's rows
  const int64_t pos = (int64_t)before + li;
  if (r < n) {
    if (lab && pos < cap) {
      idx[pos] = (int32_t)r;
      rank[r] = (int32_t)pos;
      rows[li] = (int32_t)r;
    } else {
      rank[r] = -1;
    }
  }
  if (blockIdx.x == gridDim.x - 1) {
    const int64_t total = (int64_t)before + own;
    if (tid == 0) {
      *count = (int32_t)min(total, cap);
      // the CE mean's divisor: an all-padding batch then gives the loss 0 / 1, not 0 / 0
      if (divisor) *divisor = (float)max((int64_t)1, min(total, cap));
    }
    for (int64_t i = total + tid; i < cap; i += 1024) idx[i] = -1;
  }
  __syncthreads();
  // the block's rows that fit under cap: compact rows before .. before + live - 1
  const int64_t room = cap - (int64_t)before;
  const int32_t live = room <= 0 ? 0 : (int32_t)min((int64_t)own, room);
  const int sub = lane % LPR, c0 = sub * V;
  float gm[V], bt[V];
  load_chunk<float>(gm, gamma + c0);
  load_chunk<float>(gm + 4, gamma + c0 + 4);
  load_chunk<float>(bt, beta + c0);
  load_chunk<float>(bt + 4, beta + c0 + 4);
  for (int32_t l = w * RPW + lane / LPR; l < live; l += 16 * RPW) {
    const int64_t row = rows[l], k = (int64_t)before + l;
    float v[V], o[V];
    load_chunk<__bf16>(v, X + row * ldx + c0);
    const int64_t lb = sub == 0 ? labels[row] : 0;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) s += v[j];
    const float mu = sce_group_sum<LPR>(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float u = v[j] - mu;
      q = __builtin_fmaf(u, u, q);
    }
    q = sce_group_sum<LPR>(q);
    const float rinv = 1.0f / sqrtf(q / (float)d + eps);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float u = v[j] - mu;
      o[j] = __builtin_fmaf(u * rinv, gm[j], bt[j]);
    }
    store_chunk<__bf16>(HL + k * ldh + c0, o);
    if (sub == 0) {
      lab_out[k] = lb;
      mean_out[k] = mu;
      rstd_out[k] = rinv;
    }
  }
}

// Grid-stride over all M rows, LPR lanes per row (4 waves: RPB = 256 / LPR rows per sweep).  A valid row (rank k >=
// 0) sums its `splits` slab rows in split order, rounds the sum to bf16 (the dtype the composed form stores dh in)
// and runs the LayerNorm backward of ln_bwd_v_kernel; an invalid row only writes zeros.  The affine partials of
// each lane's columns accumulate over the rows its group visits, in row order, and are combined over the
// workgroup's row groups in LDS, in group order: part[blockIdx.x][2][d].
template <int LPR>
__global__ __launch_bounds__(256) void sas_ce_rows_bwd_kernel(const float* __restrict__ slab, int splits,
                                                              int64_t slab_stride, const int32_t* __restrict__ rank,
                                                              int64_t M, const __bf16* __restrict__ X, int64_t ldx,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, __bf16* __restrict__ dX,
                                                              int64_t lddx, float* __restrict__ part) {
  constexpr int V = 8, RPW = 64 / LPR, RPB = 4 * RPW, d = LPR * V;
  const int lane = threadIdx.x & 63, sub = lane % LPR, c0 = sub * V;
  const int rgrp = (threadIdx.x >> 6) * RPW + lane / LPR;
  float pg[V], pb[V], gm[V];
  load_chunk<float>(gm, gamma + c0);
  load_chunk<float>(gm + 4, gamma + c0 + 4);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    pg[j] = 0.f;
    pb[j] = 0.f;
  }
  const int64_t stride = (int64_t)gridDim.x * RPB;
  for (int64_t row = (int64_t)blockIdx.x * RPB + rgrp; row < M; row += stride) {
    const int32_t k = rank[row];
    float o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = 0.f;
    if (k >= 0) {
      float xv[V], dy[V];
      load_chunk<__bf16>(xv, X + row * ldx + c0);
      const float mu = mean[k], a = rstd[k];
#pragma unroll
      for (int j = 0; j < V; ++j) dy[j] = 0.f;
      const float* p = slab + (int64_t)k * d + c0;
      int z = 0;
      for (; z + 4 <= splits; z += 4) {   // 4 splits' loads in flight, summed in split order (same bits)
        float4 u0[4], u1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          u0[t] = *reinterpret_cast<const float4*>(p + (int64_t)(z + t) * slab_stride);
          u1[t] = *reinterpret_cast<const float4*>(p + (int64_t)(z + t) * slab_stride + 4);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          dy[0] += u0[t].x; dy[1] += u0[t].y; dy[2] += u0[t].z; dy[3] += u0[t].w;
          dy[4] += u1[t].x; dy[5] += u1[t].y; dy[6] += u1[t].z; dy[7] += u1[t].w;
        }
      }
      for (; z < splits; ++z) {
        const float4 u0 = *reinterpret_cast<const float4*>(p + (int64_t)z * slab_stride);
        const float4 u1 = *reinterpret_cast<const float4*>(p + (int64_t)z * slab_stride + 4);
        dy[0] += u0.x; dy[1] += u0.y; dy[2] += u0.z; dy[3] += u0.w;
        dy[4] += u1.x; dy[5] += u1.y; dy[6] += u1.z; dy[7] += u1.w;
      }
      float u[V], gq[V];
      float sg = 0.f, sgu = 0.f;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        dy[j] = to_f(from_f<__bf16>(dy[j]));
        u[j] = xv[j] - mu;
        gq[j] = dy[j] * gm[j];
        pg[j] += dy[j] * (u[j] * a);
        pb[j] += dy[j];
        sg += gq[j];
        sgu += gq[j] * u[j];
      }
      sg = sce_group_sum<LPR>(sg);
      sgu = sce_group_sum<LPR>(sgu);
      const float mg = sg / (float)d;
      const float coef = a * a * a * sgu / (float)d;   // dx = a*(g - mean(g)) - coef*u
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = a * (gq[j] - mg) - coef * u[j];
    }
    store_chunk<__bf16>(dX + row * lddx + c0, o);
  }
  __shared__ float red[RPB * d];
  for (int which = 0; which < 2; ++which) {
#pragma unroll
    for (int j = 0; j < V; ++j) red[rgrp * d + c0 + j] = which == 0 ? pg[j] : pb[j];
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += 256) {
      float t = 0.f;
      for (int g = 0; g < RPB; ++g) t += red[g * d + c];
      part[((int64_t)blockIdx.x * 2 + which) * d + c] = t;
    }
    __syncthreads();
  }
}

static bool sce_al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

extern "C" {

int rs_sas_ce_rows_fwd(int dtype, int64_t M, int64_t d, const void* x, int64_t ldx, const int64_t* labels,
                       int64_t cap, const float* gamma, const float* beta, float eps, int32_t* idx, int32_t* rank,
                       int32_t* count, float* divisor, void* hl, int64_t ldh, int64_t* lab, float* mean, float* rstd,
                       void* stream) {
  if (dtype != RS_DTYPE_BF16 || (d != 64 && d != 128)) return RS_ERR_UNSUPPORTED;
  if (M <= 0 || cap <= 0 || !x || !labels || !gamma || !beta || !idx || !rank || !count || !hl || !lab || !mean ||
      !rstd || ldx < d || ldh < d || ldx % 8 || ldh % 8 || !sce_al16(x) || !sce_al16(hl) || !sce_al16(gamma) ||
      !sce_al16(beta))
    return RS_ERR_ARG;
  if (M >= ((int64_t)1 << 31)) return RS_ERR_UNSUPPORTED;
  const dim3 g((unsigned)cdiv(M, (int64_t)1024)), b(1024);
  hipStream_t s = (hipStream_t)stream;
  if (d == 64)
    hipLaunchKernelGGL((sas_ce_rows_fwd_kernel<8>), g, b, 0, s, labels, M, cap, (const __bf16*)x, ldx, gamma, beta, eps,
                       idx, rank, count, divisor, (__bf16*)hl, ldh, lab, mean, rstd);
  else
    hipLaunchKernelGGL((sas_ce_rows_fwd_kernel<16>), g, b, 0, s, labels, M, cap, (const __bf16*)x, ldx, gamma, beta,
                       eps, idx, rank, count, divisor, (__bf16*)hl, ldh, lab, mean, rstd);
  return (int)hipGetLastError();
}

int64_t rs_sas_ce_rows_nparts(int64_t M) {
  if (M <= 0) return 0;
  return std::min<int64_t>(SCE_BWD_BLOCKS, cdiv(M, (int64_t)SCE_BWD_ROWS));
}

int rs_sas_ce_rows_bwd(int dtype, int64_t M, int64_t d, const float* slab, int splits, int64_t cap,
                       const int32_t* rank, const void* x, int64_t ldx, const float* gamma, const float* mean,
                       const float* rstd, void* dx, int64_t lddx, float* part, void* stream) {
  if (dtype != RS_DTYPE_BF16 || (d != 64 && d != 128)) return RS_ERR_UNSUPPORTED;
  if (M <= 0 || cap <= 0 || splits < 1 || !slab || !rank || !x || !gamma || !mean || !rstd || !dx || !part ||
      ldx < d || lddx < d || ldx % 8 || lddx % 8 || !sce_al16(slab) || !sce_al16(x) || !sce_al16(dx) ||
      !sce_al16(gamma))
    return RS_ERR_ARG;
  const dim3 g((unsigned)rs_sas_ce_rows_nparts(M)), b(256);
  hipStream_t s = (hipStream_t)stream;
  if (d == 64)
    hipLaunchKernelGGL((sas_ce_rows_bwd_kernel<8>), g, b, 0, s, slab, splits, cap * d, rank, M, (const __bf16*)x, ldx,
                       gamma, mean, rstd, (__bf16*)dx, lddx, part);
  else
    hipLaunchKernelGGL((sas_ce_rows_bwd_kernel<16>), g, b, 0, s, slab, splits, cap * d, rank, M, (const __bf16*)x, ldx,
                       gamma, mean, rstd, (__bf16*)dx, lddx, part);
  return (int)hipGetLastError();
}

}  // extern "C"
