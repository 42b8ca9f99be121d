// torch.optim.SGD with momentum as built in BS/trainers/base.py:229-233 (args.optimizer == "SGD"): one fused sweep
// over the flat fp32 parameter buffer (gfx950, HBM-bound streaming), in the conventions of misc.hip's
// adam_step_kernel -- float4 streaming with U groups per thread, grid-stride over a bounded grid, nontemporal
// accesses for ranges far beyond the Infinity Cache, the bf16 copy of p and the transposed bf16 copies of the
// matrices the SAS backward reads.
//
//   rs_sgd_step     p, the momentum buffer (when there is one), the gradient clear, the bf16 copies; its first
//                   launch of a step also advances the step count and the dropout seed and forms the reported loss
//
// ld4 / st4 and the bf16 / transposed-store block are stream4.h's, shared with misc.hip's Adam kernels.
#include "sgd_math.h"
#include "common.h"
#include "stream4.h"
#include "../../include/recsys_hip.h"

namespace {

// one float4 of the update + its stores
template <bool BF16OUT, bool MOM, bool NT>
__device__ __forceinline__ void sgd4(int64_t i, float4 pp, float4 gg, float4 bb, float* __restrict__ p,
                                     float* __restrict__ g, float* __restrict__ buf, __bf16* __restrict__ pb,
                                     const SgdElem& h, int zero_grad, const int64_t* __restrict__ tdesc, int ntd,
                                     int64_t tbase, __bf16* __restrict__ wT, int64_t tlo, int64_t thi) {
  float* P = &pp.x; float* G = &gg.x; float* Bv = &bb.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) sgd_elem_update<MOM>(P[j], G[j], Bv[j], h);
  st4<NT>(p, i, pp);
  if (MOM) st4<NT>(buf, i, bb);
  // zero_grad: only where the gradient is not already zero (the table rows no token of the step touched)
  if (zero_grad && (__float_as_uint(gg.x) | __float_as_uint(gg.y) | __float_as_uint(gg.z) | __float_as_uint(gg.w)))
    reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (BF16OUT) {
    bf16x4 o;
    o[0] = (__bf16)P[0]; o[1] = (__bf16)P[1]; o[2] = (__bf16)P[2]; o[3] = (__bf16)P[3];
    st4_bf16_transposed<NT>(i, o, pb, tdesc, ntd, tbase, wT, tlo, thi);
  }
}

template <bool BF16OUT, bool MOM, int U, bool NT>
__global__ __launch_bounds__(256) void sgd_step_kernel(int64_t n, float* __restrict__ p, float* __restrict__ g,
                                                       float* __restrict__ buf, __bf16* __restrict__ pb,
                                                       double* state, const double* __restrict__ hyper,
                                                       int zero_grad, int prepare, const float* __restrict__ divisor,
                                                       uint64_t* seed_base, const int64_t* __restrict__ tdesc,
                                                       int ntd, int64_t tbase, __bf16* __restrict__ wT,
                                                       const float* __restrict__ lsum, float* lout) {
  // the step's bookkeeping by one thread: nothing in this kernel reads any of the three, so no workgroup has to
  // wait for another (unlike the Adam launch, whose scalars depend on the step count)
  if (prepare && blockIdx.x == 0 && threadIdx.x == 0) {
    state[0] += 1.0;
    if (seed_base) *seed_base += 1;
    if (lout) *lout = lsum[0] / divisor[0];
  }
  const SgdElem h = sgd_elem(hyper, divisor);
  int64_t tlo = 0, thi = 0;
  if (BF16OUT && ntd > 0) {
    tlo = INT64_MAX;
    for (int k = 0; k < ntd; ++k) {
      const int64_t* dk = tdesc + 6 * k;
      tlo = min(tlo, dk[2]);
      thi = max(thi, dk[2] + dk[0] * dk[3]);
    }
  }
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // U float4 per thread in flight: every load of the group is issued before the first store
  for (; i + (U - 1) * stride < n4; i += U * stride) {
    float4 pq[U], gq[U], bq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      pq[u] = ld4<NT>(p, i + u * stride);
      gq[u] = ld4<NT>(g, i + u * stride);
      bq[u] = MOM ? ld4<NT>(buf, i + u * stride) : z4;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      sgd4<BF16OUT, MOM, NT>(i + u * stride, pq[u], gq[u], bq[u], p, g, buf, pb, h, zero_grad, tdesc, ntd, tbase, wT,
                             tlo, thi);
  }
  for (; i < n4; i += stride) {
    const float4 pp = ld4<NT>(p, i);
    const float4 gg = ld4<NT>(g, i);
    const float4 bb = MOM ? ld4<NT>(buf, i) : z4;
    sgd4<BF16OUT, MOM, NT>(i, pp, gg, bb, p, g, buf, pb, h, zero_grad, tdesc, ntd, tbase, wT, tlo, thi);
  }
  // tail
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t j = n4 * 4 + threadIdx.x;
    float P = p[j], B = MOM ? buf[j] : 0.f;
    sgd_elem_update<MOM>(P, g[j], B, h);
    p[j] = P;
    if (MOM) buf[j] = B;
    if (BF16OUT) pb[j] = (__bf16)P;
    if (zero_grad) g[j] = 0.f;
  }
}

}  // namespace

// two float4 groups in flight per thread and the nontemporal threshold: misc.hip's (ADAM_NT_MIN), measured there
#define SGD_U 2
#define SGD_NT_MIN (64ll << 20)
#define SGD_LAUNCH(BO, MO)                                                                                     \
  do {                                                                                                         \
    if (n >= SGD_NT_MIN)                                                                                       \
      hipLaunchKernelGGL((sgd_step_kernel<BO, MO, SGD_U, true>), dim3((unsigned)blocks), dim3(256), 0, s, n, p, g, \
                         buf, (__bf16*)p_bf16, state, hyper, zero_grad, prepare, grad_divisor, seed_base, tdesc, ntd, \
                         tbase, (__bf16*)wT, loss_sum, loss_out);                                              \
    else                                                                                                       \
      hipLaunchKernelGGL((sgd_step_kernel<BO, MO, SGD_U, false>), dim3((unsigned)blocks), dim3(256), 0, s, n, p, g, \
                         buf, (__bf16*)p_bf16, state, hyper, zero_grad, prepare, grad_divisor, seed_base, tdesc, ntd, \
                         tbase, (__bf16*)wT, loss_sum, loss_out);                                              \
  } while (0)

extern "C" {

int rs_sgd_step(int64_t n, float* p, float* g, float* buf, void* p_bf16, double* state, const double* hyper,
                int zero_grad, int prepare, const float* grad_divisor, uint64_t* seed_base, const int64_t* tdesc,
                int ntd, int64_t tbase, void* wT, const float* loss_sum, float* loss_out, int max_wg, void* stream) {
  if (n <= 0 || !p || !g || !state || !hyper || max_wg < 0) return RS_ERR_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) % 16 || (uintptr_t)p_bf16 % 8) return RS_ERR_ARG;
  if (ntd < 0 || (ntd > 0 && (!tdesc || !wT || !p_bf16))) return RS_ERR_ARG;
  if (loss_out && (!loss_sum || !grad_divisor)) return RS_ERR_ARG;
  int64_t blocks = std::max<int64_t>(1, cdiv(n / 4, 256));
  if (max_wg > 0) blocks = std::min<int64_t>(blocks, max_wg);
  if (blocks > 0x7fffffffll) return RS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (p_bf16) {
    if (buf) SGD_LAUNCH(true, true);
    else SGD_LAUNCH(true, false);
  } else {
    if (buf) SGD_LAUNCH(false, true);
    else SGD_LAUNCH(false, false);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
