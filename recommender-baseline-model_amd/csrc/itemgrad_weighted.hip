// rs-build: included by grad_tail.hip (compiled once, as part of that translation unit, after itemgrad.hip)
// The weighted form of the inverted-index item-table gradient: one weight per entry, `per` entries per source row
// (rs_item_grad_weighted).  It uses itemgrad.hip's index layout, GradArgs and span pass, and is included last so that
// no other kernel of the translation unit moves.
// Over an index built by rs_item_index_build(1, keys, rows * per, ...): entry e of the keys belongs to source row
// e / per and carries the weight w[e]; dtable[key_e] += sum_e w[e] * f[e / per].  The chunk structure, the summation
// order and the span pass are item_chunk_f32_kernel's / item_span_f32_kernel's: one workgroup per chunk of CH sorted
// entries sums each key run in sorted-entry order, a run crossing the chunk's edge leaves a partial in the chunk's slot,
// and item_span_f32_kernel adds a crossing run's partials in chunk order.  Nothing of size entries x d is formed: a
// term is w[e] * f[row][c] on the fly.  Key 0 is skipped (its weight and row are not read).
namespace ig {
struct WeightedArgs {
  const void* f;
  int64_t ldf;
  const float* w;
  uint32_t per;
};

template <typename T>
__global__ __launch_bounds__(256) void item_chunk_weighted_kernel(GradArgs a, WeightedArgs wa, int64_t d) {
  static_assert(CH + 2 <= 64, "item_chunk_weighted_kernel: the sentinel threads must exist at 64 threads per workgroup");
  __shared__ uint32_t skey[CH + 2];   // [0]: the key before the chunk, [1 .. cnt]: the chunk's, [cnt + 1]: the next
  __shared__ int sm_m[CH];
  __shared__ float sm_w[CH];
  const int tid = threadIdx.x;
  const int64_t chunk = blockIdx.x, base = chunk * CH;
  const int cnt = (int)min((int64_t)CH, a.n - base);
  if (tid < cnt) {
    const uint32_t k = a.sk[base + tid], ent = a.sv[base + tid];
    skey[tid + 1] = k;
    sm_m[tid] = k ? (int)(ent / wa.per) : -1;
    sm_w[tid] = k ? wa.w[ent] : 0.f;
  }
  if (tid == CH) skey[0] = base > 0 ? a.sk[base - 1] : 0xffffffffu;
  if (tid == CH + 1) skey[cnt + 1] = base + cnt < a.n ? a.sk[base + cnt] : 0xffffffffu;
  __syncthreads();
  const T* f = (const T*)wa.f;
  for (int64_t c = tid; c < d; c += blockDim.x) {
    float raw[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      raw[j] = 0.f;
      if (j < cnt && sm_m[j] >= 0) raw[j] = to_f(f[(int64_t)sm_m[j] * wa.ldf + c]);
    }
    float acc = 0.f;
    int rs = 0;                               // the current run's first entry in the chunk
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      if (j < cnt) {
        acc += sm_w[j] * raw[j];
        const uint32_t k = skey[j + 1];
        if (j + 1 == cnt || skey[j + 2] != k) {        // the run ends at entry j of this chunk
          if (k != 0) {                                 // padding_idx 0: no gradient
            const bool from_before = rs == 0 && skey[0] == k;
            const bool past_end = j + 1 == cnt && skey[cnt + 1] == k;
            if (!from_before && !past_end) a.dtable[(int64_t)k * d + c] += acc;
            else a.part[(chunk * 2 + (rs == 0 ? 0 : 1)) * d + c] = acc;
          }
          acc = 0.f;
          rs = j + 1;
        }
      }
    }
  }
}
}  // namespace ig

extern "C" int rs_item_grad_weighted(const void* ws, int dtype, int64_t rows, int64_t per, int64_t table_rows,
                                     int64_t d, const void* f, int64_t ldf, const float* w, float* dtable,
                                     void* stream) {
  if (dtype != RS_DTYPE_F32 && dtype != RS_DTYPE_BF16) return RS_ERR_UNSUPPORTED;
  if (rows <= 0 || per <= 0 || rows * per >= ((int64_t)1 << 31) || table_rows <= 0 || d <= 0 || !ws || !f || !w ||
      !dtable || ldf < d)
    return RS_ERR_ARG;
  ig::Layout L;
  hipError_t e = ig::layout(1, rows * per, table_rows, d, L);
  if (e != hipSuccess) return (int)e;
  if (table_rows < 2) return 0;
  const char* p = (const char*)ws;
  ig::GradArgs a = {};
  a.sk = (const uint32_t*)(p + L.sk);
  a.sv = (const uint32_t*)(p + L.sv);
  a.part = (float*)(p + L.part);
  a.n = L.n;
  a.rows = L.n;
  a.dtable = dtable;
  a.start = L.cs ? (const int*)(p + L.start) : nullptr;
  const ig::WeightedArgs wa = {f, ldf, w, (uint32_t)per};
  hipStream_t s = (hipStream_t)stream;
  const int64_t nch = cdiv(L.n, ig::CH);
  const dim3 block(d > 128 ? 256 : (d > 64 ? 128 : 64));
  if (dtype == RS_DTYPE_BF16)
    hipLaunchKernelGGL(ig::item_chunk_weighted_kernel<__bf16>, dim3((unsigned)nch), block, 0, s, a, wa, d);
  else
    hipLaunchKernelGGL(ig::item_chunk_weighted_kernel<float>, dim3((unsigned)nch), block, 0, s, a, wa, d);
  hipLaunchKernelGGL(ig::item_span_f32_kernel, dim3((unsigned)cdiv(nch, 4)), dim3(256), 0, s, a, nch, d);
  return (int)hipGetLastError();
}
