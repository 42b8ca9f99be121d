// Helpers of the optimizer sweeps (misc.hip's Adam kernels, sgd.hip): streaming float4 access and the transposed bf16
// stores of the matrices inside the flat buffer.  One definition for both units.
#pragma once
#include "common.h"

// streaming float4 access; NT: nontemporal (slc / nt) loads and stores for the optimizer's single-use sweeps
typedef float f4v __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4 ld4(const float* a, int64_t i) {
  if (NT) {
    const f4v x = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(a) + i);
    return make_float4(x[0], x[1], x[2], x[3]);
  }
  return reinterpret_cast<const float4*>(a)[i];
}
template <bool NT>
__device__ __forceinline__ void st4(float* a, int64_t i, float4 v) {
  if (NT) {
    const f4v x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<f4v*>(a) + i);
  } else {
    reinterpret_cast<float4*>(a)[i] = v;
  }
}

// the bf16 copy of float4 i, then its transposed copies (the SAS backward's [in][out] block weights,
// rs_transpose_bf16's desc layout): the 4 elements share a row (host checks lds % 4 == 0)
template <bool NT>
__device__ __forceinline__ void st4_bf16_transposed(int64_t i, bf16x4 o, __bf16* __restrict__ pb,
                                                    const int64_t* __restrict__ tdesc, int ntd, int64_t tbase,
                                                    __bf16* __restrict__ wT, int64_t tlo, int64_t thi) {
  if (NT) {
    uint64_t w;
    __builtin_memcpy(&w, &o, 8);
    __builtin_nontemporal_store(w, reinterpret_cast<uint64_t*>(pb) + i);
  } else {
    reinterpret_cast<bf16x4*>(pb)[i] = o;
  }
  // the descriptors' element span [tlo, thi) first: most of the buffer (the tables) is outside every matrix
  const int64_t e0 = tbase + 4 * i;
  const int nk = (e0 >= tlo && e0 < thi) ? ntd : 0;
  for (int k = 0; k < nk; ++k) {
    const int64_t* dk = tdesc + 6 * k;
    const int64_t rel = tbase + 4 * i - dk[2];
    if (rel >= 0 && rel < dk[0] * dk[3]) {
      // 32-bit division (a weight matrix: rows * row stride < 2^31, host-checked); the 64-bit one is a
      // ~60-instruction sequence per float4 of every transposed weight
      const uint32_t ru = (uint32_t)rel, ld = (uint32_t)dk[3];
      const int64_t r = ru / ld, c = ru - (uint32_t)r * ld;
      if (c < dk[1]) {
        __bf16* t = wT + dk[4] + c * dk[5] + r;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j * dk[5]] = o[j];
      }
    }
  }
}
