// On-device evaluation loader (gfx950): the per-user test negatives and the evaluation batches.
//
// rs_eval_negatives replaces the reference's negative samplers (BS/dataloaders/negative_samplers/random.py:18-35,
// popular.py:25-42): per user a Python rejection loop over np.random.choice.  Here user u owns a raw draw stream
//   x(u, c) = item_of( splitmix64( splitmix64(seed ^ (A * (u + 1))) + C * (c + 1) ) ),   c = 0, 1, ...
// (A = 0xA0761D6478BD642F, C = 0x632BE59BD9B4E019; item_of: uniform over [1, item_num] or the alias rule of
// rs_alias_items, see the header) and negs[u] = that stream with every item of seen(u) and every repeat of an earlier
// kept item dropped, the first n_neg survivors in stream order -- RandomNegativeSampler's
// `while item in seen or item in samples` loop run on that stream.  The stream is a function of (seed, u, c) alone, so
// the result does not depend on how the users are split over launches.
//
// One wave per user, four per workgroup, 64 draws per round: every lane binary-searches the user's sorted seen list
// (global memory), probes the wave's LDS open-addressing table of kept items, a repeat inside the round is given to the
// lower lane, and a ballot + prefix popcount hands out the output slots.  No loop is unbounded: at most MAX_DRAWS raw
// draws per user, then the open slots take the smallest ids that are neither seen nor kept (a scan bounded by
// item_num).
//
// rs_eval_batch builds SASEvalDataset / BertEvalDataset's rows (BS/dataloaders/sas.py:136-153, bert.py:128-142) for a
// range of users: the history's tail (+ the validation item in test mode, + [MASK] for BERT), left padded;
// candidates = {answer, negatives}; labels = {1, 0, ...}.
#include "common.h"
#include "../../include/recsys_hip.h"

namespace evl {

constexpr int NEGS_MAX = 1024;     // rs_eval_negs_max()
constexpr int MAX_DRAWS = 4096;    // rs_eval_negatives_max_draws(): 64 rounds of 64
constexpr int MAX_LEN = 512;       // rs_eval_batch's max_len bound (the samplers' bound)
constexpr int WAVES = 4;

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t user_key(uint64_t seed, int64_t u) {
  return splitmix64(seed ^ (0xA0761D6478BD642Full * (uint64_t)(u + 1)));
}

// raw draw c of the user with key `key`: an item id in [1, item_num]
__device__ __forceinline__ int32_t draw(uint64_t key, int64_t c, uint64_t item_num, const uint64_t* __restrict__ table) {
  const uint64_t r = splitmix64(key + 0x632BE59BD9B4E019ull * (uint64_t)(c + 1));
  const uint64_t slot = __umul64hi(r, item_num);                    // < item_num
  if (!table) return (int32_t)slot + 1;
  const uint32_t frac = (uint32_t)((r * item_num) >> 32);
  const uint64_t e = table[slot];
  return frac < (uint32_t)e ? (int32_t)slot + 1 : (int32_t)(e >> 32);
}

__device__ __forceinline__ bool in_seen(const int32_t* __restrict__ seen, int64_t lo, int64_t hi, int32_t v) {
  while (lo < hi) {                                                 // <= 32 steps
    const int64_t mid = (lo + hi) >> 1;
    const int32_t x = seen[mid];
    if (x == v) return true;
    if (x < v) lo = mid + 1; else hi = mid;
  }
  return false;
}

__device__ __forceinline__ int slot_of(int32_t v, int mask) { return (int)(((uint32_t)v * 0x9E3779B1u) >> 7) & mask; }

// kept items: open addressing over hs = mask + 1 slots, 0 = empty; at most n_neg <= hs / 2 entries, so a probe ends
__device__ __forceinline__ bool in_kept(const int32_t* tab, int mask, int32_t v) {
  int s = slot_of(v, mask);
  for (int p = 0; p <= mask; ++p) {
    const int32_t x = tab[s];
    if (x == v) return true;
    if (x == 0) return false;
    s = (s + 1) & mask;
  }
  return false;
}

__device__ __forceinline__ void keep(int32_t* tab, int mask, int32_t v) {
  int s = slot_of(v, mask);
  for (int p = 0; p <= mask; ++p) {
    if (atomicCAS(&tab[s], 0, v) == 0) return;
    s = (s + 1) & mask;
  }
}

// the lanes of one wave exchange data through their LDS table: order the table's writes before the reads that follow
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(256) void negatives_kernel(const int64_t* __restrict__ seen_off,
                                                        const int32_t* __restrict__ seen, int64_t user0, int64_t count,
                                                        int64_t item_num, int n_neg, int hs, uint64_t seed,
                                                        const uint64_t* __restrict__ table, int32_t* __restrict__ negs,
                                                        int32_t* __restrict__ n_drawn, int64_t* __restrict__ draws) {
  extern __shared__ int32_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * WAVES + wave;
  if (i >= count) return;                                           // the whole wave; no workgroup barrier below
  const int64_t u = user0 + i;
  int32_t* tab = lds + wave * hs;
  const int mask = hs - 1;
  for (int s = lane; s < hs; s += 64) tab[s] = 0;
  wave_sync();
  const uint64_t key = user_key(seed, u);
  const int64_t s_lo = seen_off[u], s_hi = seen_off[u + 1];
  int32_t* out = negs + u * n_neg;
  if (draws)
    for (int c = lane; c < MAX_DRAWS; c += 64) draws[u * MAX_DRAWS + c] = draw(key, c, (uint64_t)item_num, table);
  const uint64_t below = (1ull << lane) - 1ull;
  int kept = 0, drawn = 0;
  for (int round = 0; round < MAX_DRAWS / 64 && kept < n_neg; ++round) {
    const int32_t v = draw(key, (int64_t)round * 64 + lane, (uint64_t)item_num, table);
    bool ok = !in_seen(seen, s_lo, s_hi, v) && !in_kept(tab, mask, v);
    for (int j = 0; j < 63; ++j) {                                  // a repeat inside the round: the lower lane wins
      const int32_t vj = __shfl(v, j, 64);
      if (j < lane && vj == v) ok = false;
    }
    const uint64_t m = __ballot(ok);
    const int slot = kept + __popcll(m & below);
    if (ok && slot < n_neg) {
      out[slot] = v;
      keep(tab, mask, v);
    }
    const int got = __popcll(m);
    if (kept + got >= n_neg) {                                      // the lane that filled the last slot ends the stream
      const uint64_t last = __ballot(ok && slot == n_neg - 1);
      drawn = round * 64 + (__ffsll((unsigned long long)last) - 1) + 1;
      kept = n_neg;
    } else {
      kept += got;
    }
    wave_sync();
  }
  if (kept < n_neg) {
    // MAX_DRAWS raw draws did not fill the row: the smallest ids neither seen nor kept, ascending
    const int before = kept;
    for (int64_t base = 0; base < item_num && kept < n_neg; base += 64) {
      const int64_t v = base + lane + 1;
      const bool ok = v <= item_num && !in_seen(seen, s_lo, s_hi, (int32_t)v) && !in_kept(tab, mask, (int32_t)v);
      const uint64_t m = __ballot(ok);
      const int slot = kept + __popcll(m & below);
      if (ok && slot < n_neg) out[slot] = (int32_t)v;
      kept = min(n_neg, kept + __popcll(m));
    }
    drawn = -1 - (kept - before);
    for (int s = kept + lane; s < n_neg; s += 64) out[s] = 0;       // only if the caller broke its promise
  }
  if (n_drawn && lane == 0) n_drawn[u] = drawn;
}

__global__ __launch_bounds__(256) void batch_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ items,
                                                    const int64_t* __restrict__ extra,
                                                    const int64_t* __restrict__ answer,
                                                    const int32_t* __restrict__ negs, int64_t user0, int T, int n_neg,
                                                    int64_t mask_token, int64_t* __restrict__ seq,
                                                    int64_t* __restrict__ cand, int64_t* __restrict__ labels) {
  const int64_t b = blockIdx.x, u = user0 + b;
  const int64_t s0 = off[u], L = off[u + 1] - s0;
  const int64_t full = L + (extra ? 1 : 0) + (mask_token > 0 ? 1 : 0);   // history (+ validation item) (+ [MASK])
  for (int t = threadIdx.x; t < T; t += 256) {
    const int64_t j = full - T + t;                                 // position in the extended history
    int64_t v = 0;
    if (j >= 0) v = j < L ? items[s0 + j] : (j == L && extra ? extra[u] : mask_token);
    seq[b * T + t] = v;
  }
  const int C = 1 + n_neg;
  for (int c = threadIdx.x; c < C; c += 256) {
    cand[b * C + c] = c == 0 ? answer[u] : (int64_t)negs[u * n_neg + c - 1];
    labels[b * C + c] = c == 0 ? 1 : 0;
  }
}

}  // namespace evl

extern "C" {

int64_t rs_eval_negs_max(void) { return evl::NEGS_MAX; }
int64_t rs_eval_negatives_max_draws(void) { return evl::MAX_DRAWS; }

int rs_eval_negatives_draws(const int64_t* seen_offsets, const int32_t* seen_sorted, int64_t user0, int64_t count,
                            int64_t item_num, int64_t n_neg, uint64_t seed, const uint64_t* table, int32_t* negs,
                            int32_t* n_drawn, int64_t* draws, void* stream) {
  if (!seen_offsets || !seen_sorted || !negs || user0 < 0 || count < 1 || item_num < 1 ||
      item_num >= ((int64_t)1 << 31) || n_neg < 1 || n_neg > evl::NEGS_MAX || n_neg > item_num)
    return RS_ERR_ARG;
  int hs = 64;
  while (hs < 2 * n_neg) hs *= 2;                                   // <= 2048 slots: 8 KiB per wave
  hipLaunchKernelGGL(evl::negatives_kernel, dim3((unsigned)cdiv(count, (int64_t)evl::WAVES)), dim3(256),
                     (size_t)evl::WAVES * hs * sizeof(int32_t), (hipStream_t)stream, seen_offsets, seen_sorted, user0,
                     count, item_num, (int)n_neg, hs, seed, table, negs, n_drawn, draws);
  return (int)hipGetLastError();
}

int rs_eval_negatives(const int64_t* seen_offsets, const int32_t* seen_sorted, int64_t user0, int64_t count,
                      int64_t item_num, int64_t n_neg, uint64_t seed, const uint64_t* table, int32_t* negs,
                      int32_t* n_drawn, void* stream) {
  return rs_eval_negatives_draws(seen_offsets, seen_sorted, user0, count, item_num, n_neg, seed, table, negs, n_drawn,
                                 nullptr, stream);
}

int rs_eval_batch(const int64_t* hist_offsets, const int64_t* hist_items, const int64_t* extra, const int64_t* answer,
                  const int32_t* negs, int64_t user0, int64_t B, int64_t max_len, int64_t n_neg, int64_t mask_token,
                  int64_t* seq, int64_t* cand, int64_t* labels, void* stream) {
  if (!hist_offsets || !hist_items || !answer || !negs || !seq || !cand || !labels || user0 < 0 || B < 1 ||
      max_len < 1 || max_len > evl::MAX_LEN || n_neg < 1 || n_neg > evl::NEGS_MAX || mask_token < 0)
    return RS_ERR_ARG;
  hipLaunchKernelGGL(evl::batch_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, hist_offsets, hist_items,
                     extra, answer, negs, user0, (int)max_len, (int)n_neg, mask_token, seq, cand, labels);
  return (int)hipGetLastError();
}

}  // extern "C"
