// torch.optim.SGD's per-element update (BS/trainers/base.py:229-233: optim.SGD(params, lr, weight_decay=...,
// momentum=...); dampening = 0, nesterov = False; the single-tensor path of torch/optim/sgd.py) for the optimizer
// sweep (sgd.hip): one definition, every rounding spelled out, so any kernel that inlines it produces the same bits.
#pragma once
#include "common.h"

// The hyperparameters are Python doubles in torch and meet the fp32 tensors as floats: hyper is double[3] =
// {lr, momentum, weight_decay}, each cast here.  gs = 1 / the data-parallel count (1 without one).
struct SgdElem { float lr, mom, wd, gs; };
__device__ __forceinline__ SgdElem sgd_elem(const double* hyper, const float* divisor) {
  return {(float)hyper[0], (float)hyper[1], (float)hyper[2], divisor ? 1.f / divisor[0] : 1.f};
}
// one element: gradient scale, weight decay grad.add(param, alpha=wd) (one fma), buf.mul_(momentum).add_(grad) (TWO
// roundings: torch runs them as two kernels, so no fma), param.add_(buf, alpha=-lr) (one fma).  A zero-initialised
// buffer gives torch's first-step rule buf = grad.clone() from the same line (0 * mom + g; only the sign of a zero
// buffer element can differ, and that never reaches P).  MOM = false: no buffer, param.add_(grad, alpha=-lr).
// No contraction but the spelled-out ones: the three other fma / no-fma choices of the decay and update lines each
// differ from torch's CPU float32 SGD in thousands of 100k elements after 20 steps.
template <bool MOM>
__device__ __forceinline__ void sgd_elem_update(float& P, float G, float& B, const SgdElem& h) {
#pragma clang fp contract(off)
  float gj = h.gs == 1.f ? G : G * h.gs;
  if (h.wd != 0.f) gj = __builtin_fmaf(h.wd, P, gj);
  if (MOM) {
    B = (B * h.mom) + gj;
    gj = B;
  }
  P = __builtin_fmaf(-h.lr, gj, P);
}
