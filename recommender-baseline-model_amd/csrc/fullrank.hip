// Full-catalogue ranking and top-K: one vocabulary-tile-stationary sweep over every item, no score matrix (gfx950).
//
// Reference: the trainers score a hand-picked candidate list (BS/trainers/sas.py:56-62, BS/trainers/bert.py:43-52)
// and rank it with recalls_ndcgs_and_mrr_for_ks (BS/trainers/utils.py:28-57).  Here the candidates are every item:
//   s(b, v) = fp32(sum_k h[b][k] E[v][k]) (+ bias[v]),   A(b) = {v_lo <= v < v_hi, v not in excl[b]},
//   v before w  <=>  s_v > s_w or (s_v == s_w and v < w),
// rs_full_rank counts the admissible items before the target, rs_full_topk returns the first K of A(b).  A dense
// (B, V) fp32 score matrix is 1 GB at B = 256, V = 1M; nothing of it is formed here.
//
// Shape (vocab_head.hip's): workgroup x owns the 128-item vocabulary tiles x, x + gridDim.x, ...; an E tile sits in
// LDS (bf16: whole, zero-padded in k to a multiple of 32, so any d <= 256 runs the same code) while every 128-row tile
// of h is multiplied against it.  S^T = E_tile . h_tile^T is accumulated transposed: lane (g = lane >> 4,
// cl = lane & 15) of wave (wm, wn) holds acc[i][j][r] = s(row 64 wn + 16 j + cl, item 32 wm + 16 i + 4 g + r), i.e.
// consecutive items of one row, so the per-row count / filter reduces in registers.  fp32 (the parity dtype) runs the
// same tile routine on the exact f32 MFMA with 32-deep k chunks staged through LDS (E re-read per row tile: slow, and
// meant to be).
//
// Three modes of one kernel, so that every score comes out of the same instructions in the same k order:
//   TGT   workgroup b forms the tile that holds target[b] against b's row tile and keeps s(b, target[b]).  An item
//         whose E row and bias equal the target's then ties with it bit for bit in the sweep, and ids decide.
//   RANK  per accumulator: admissible, not the target, before the target?  Counts reduce per row over the lane's 8
//         items and the 4 lane groups, then one LDS atomic per (wave, row); a workgroup adds its per-row totals to
//         rank[b] with one integer atomic each at its end (order-independent: deterministic).
//   TOPK  threshold filter.  Per (workgroup, row) the workspace keeps a survivor list of CAP = max(2K, 32) keys and
//         the threshold (the K-th best key at the last compaction).  key = (order-preserving bits of s) << 32 |
//         ~id, so "before" is "greater key" and keys are distinct.  A key above the threshold takes a slot by an LDS
//         atomic on the row's count; when a list is full the owning workgroup keeps its K best (rank by counting, a
//         wave per row, keys in registers) and raises the threshold; lanes that found no slot try again.  Any input
//         order is correct; ascending scores only compact more often.  At the end each list is sorted, and a second
//         launch merges the <= 256 lists of a row (K rounds of a block-wide max over the list heads).
// Admissibility costs no probe per score: per (row tile, vocabulary tile) one thread per row binary-searches the
// row's SORTED exclusion list for the tile's id range and sets bits in a [128][128]-bit LDS mask; a lane then tests
// one bit per score.  excl == NULL skips all of it.
// No workgroup waits for another: the sweep and the merge are separate launches.
#include "common.h"
#include "../../include/recsys_hip.h"
#include <type_traits>

namespace fr {
typedef __bf16 bf16;
typedef unsigned long long u64;
typedef __attribute__((ext_vector_type(4))) unsigned u4;

constexpr int BV = 128, BR = 128, NTH = 512, FV = 2;
constexpr int NSL = 256;          // most vocabulary slices (workgroups along x) of a launch
constexpr int BCAP = 4096;        // RANK: rows whose counts a workgroup keeps in LDS (more rows: global atomics)
constexpr int PAD = 8;            // bf16 elements of padding per LDS row (16 rows of a fragment -> 16 bank groups)
constexpr int FK = 32, FP = 36;   // fp32: k-chunk depth and LDS row pitch (floats)
enum { TGT = 0, RANK = 1, TOPK = 2 };

struct Args {
  const void* h; int64_t ldh;
  const void* E; int64_t lde;
  const float* bias;
  int64_t B; int d, dkp;
  int64_t v_lo, v_hi;
  const int64_t* target;
  const int64_t* excl; int64_t nx, ldx;
  int* rank;                 // TGT: 0 / -1; RANK: += count
  float* ts;                 // target scores (workspace)
  float* ts_out;             // nullable copy for the caller
  int K, cap;
  u64* thr; int* cnt; u64* lists;   // TOPK state [slice][B] (, [cap])
  int vec_h, vec_e;          // 16-B loads allowed
};

__host__ __device__ inline int cap_of(int K) { return 2 * K > 32 ? 2 * K : 32; }

// TOPK state in the workspace is written and read by ONE workgroup for the whole launch (the merge is a later
// launch): workgroup-scope accesses ordered by the workgroup's barriers -- no agent-scope fence, which on gfx950
// writes back and invalidates the L2 that holds h and the other workgroups' lists
__device__ __forceinline__ u64 ld_u64(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_u64(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int ld_i32(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_i32(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m, 64), hi = __shfl_xor((unsigned)(v >> 32), m, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_max64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = shfl_xor64(v, o);
    v = w > v ? w : v;
  }
  return v;
}

// greater key <=> earlier in the total order (finite scores; -0 was folded into +0 by the caller)
__device__ __forceinline__ u64 make_key(float s, int v) {
  const unsigned b = __builtin_bit_cast(unsigned, s);
  const unsigned o = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
  return ((u64)o << 32) | (u64)(0xffffffffu - (unsigned)v);
}
__device__ __forceinline__ void split_key(u64 key, float& s, int64_t& v) {
  const unsigned o = (unsigned)(key >> 32);
  const unsigned b = o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu);
  s = __builtin_bit_cast(float, b);
  v = (int64_t)(0xffffffffu - (unsigned)key);
}

// score of a threshold key (0: nothing kept yet, every finite score passes)
__device__ __forceinline__ float key_score(u64 key) {
  float s;
  int64_t v;
  split_key(key, s, v);
  return key == 0ull ? -__builtin_inff() : s;
}

// One wave: keep the min(n, K) greatest of list[0 .. n) (n <= 256, distinct keys), sorted descending, in
// list[0 .. min(n, K)); returns the K-th greatest (0 when n < K).  Keys live in registers (4 per lane).
__device__ __forceinline__ u64 compact(u64* list, int n, int K, int lane) {
  u64 k[4];
  int rk[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) k[q] = (lane + 64 * q < n) ? ld_u64(list + lane + 64 * q) : 0ull;
#pragma unroll
  for (int q2 = 0; q2 < 4; ++q2) {
    if (q2 * 64 < n) {
      const int m = min(64, n - q2 * 64);
      for (int l = 0; l < m; ++l) {
        const u64 kf = shfl64(k[q2], l);
#pragma unroll
        for (int q = 0; q < 4; ++q) rk[q] += kf > k[q] ? 1 : 0;
      }
    }
  }
  u64 kth = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool live = lane + 64 * q < n;
    if (live && rk[q] < K) st_u64(list + rk[q], k[q]);
    if (live && rk[q] == K - 1) kth = k[q];
  }
  return wave_max64(kth);
}

// The same for four lists of at most 64 keys (one per lane), the loads of all four in flight together: a wave
// compacts its rows one after another, and each list costs an L2 round trip.  kth[c]: as compact's return.
__device__ __forceinline__ void compact4(u64* const (&list)[4], const int (&n)[4], int K, int lane, u64 (&kth)[4]) {
  u64 k[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) k[c] = lane < n[c] ? ld_u64(list[c] + lane) : 0ull;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    kth[c] = 0ull;
    if (n[c] > 0) {                          // wave-uniform
      int rk = 0;
      for (int l = 0; l < n[c]; ++l) rk += shfl64(k[c], l) > k[c] ? 1 : 0;
      const bool live = lane < n[c];
      if (live && rk < K) st_u64(list[c] + rk, k[c]);
      kth[c] = wave_max64(live && rk == K - 1 ? k[c] : 0ull);
    }
  }
}

// LDS image [128][dkp + PAD] of rows r0 .. r0 + 127 of src (rows >= rend and columns >= d read as zero).  vec: rows
// are 16-B loadable (d % 8 == 0 then): dkp / 32 chunks per thread, 4 in flight; else element by element
__device__ __forceinline__ void fill_tile(bf16* dst, const bf16* src, int64_t r0, int64_t rend, int64_t ld, bool vec, int d,
                                          int dkp, int tid) {
  const int P = dkp + PAD;
  if (vec) {
    const int cpr = dkp >> 3, nch = dkp >> 5;
    for (int c0 = 0; c0 < nch; c0 += 4) {
      u4 x[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ch = tid + NTH * (c0 + c), r = ch / cpr, k8 = (ch - r * cpr) * 8;
        x[c] = (u4){0u, 0u, 0u, 0u};
        if (c0 + c < nch && r0 + r < rend && k8 < d) x[c] = *reinterpret_cast<const u4*>(src + (r0 + r) * ld + k8);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ch = tid + NTH * (c0 + c), r = ch / cpr, k8 = (ch - r * cpr) * 8;
        if (c0 + c < nch) *reinterpret_cast<u4*>(dst + r * P + k8) = x[c];
      }
    }
  } else {
    for (int idx = tid; idx < BR * dkp; idx += NTH) {
      const int r = idx / dkp, k = idx - r * dkp;
      dst[r * P + k] = (r0 + r < rend && k < d) ? src[(r0 + r) * ld + k] : (bf16)0.0f;
    }
  }
}
__device__ __forceinline__ void load8(float* o, const float* row, int k8, int d, bool vec, bool live) {
  if (vec) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (live && k8 < d) {
      a = *reinterpret_cast<const float4*>(row + k8);
      b = *reinterpret_cast<const float4*>(row + k8 + 4);
    }
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (live && k8 + e < d) ? row[k8 + e] : 0.f;
  }
}

template <typename T> __host__ __device__ inline int tile_bytes(int dkp) {
  return std::is_same<T, float>::value ? BR * FP * 4 : BR * (dkp + PAD) * 2;
}
template <typename T, int MODE> __host__ __device__ inline int lds_bytes(int dkp) {
  return 2 * tile_bytes<T>(dkp) + BR * 4 * 4 /* mask */ + BR * 8 /* thr */ + BR * 4 /* tgt | cnt */ + BR * 4 /* ts */ +
         (MODE == RANK ? BCAP * 4 : 0);
}

template <typename T, int MODE>
__global__ __launch_bounds__(NTH, 1) void sweep_kernel(Args a) {
  constexpr bool F32 = std::is_same<T, float>::value;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tb = tile_bytes<T>(a.dkp);
  T* Et = reinterpret_cast<T*>(smem);
  T* Hs = reinterpret_cast<T*>(smem + tb);
  u64* thrL = reinterpret_cast<u64*>(smem + 2 * tb);
  unsigned* msk = reinterpret_cast<unsigned*>(thrL + BR);     // [BR][4]
  int* metaL = reinterpret_cast<int*>(msk + BR * 4);          // RANK / TGT: target id (-1: none); TOPK: list count
  float* tsL = reinterpret_cast<float*>(metaL + BR);
  int* accL = reinterpret_cast<int*>(tsL + BR);               // RANK: [BCAP]

  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
  const int v0w = wm * 32;
  const int P = a.dkp + PAD;
  const int64_t B = a.B;
  const int nrt = (int)cdiv(B, BR);
  const int64_t nvt = cdiv(a.v_hi - a.v_lo, BV);
  const bool has_ex = MODE != TGT && a.excl != nullptr && a.nx > 0;
  const bool lds_cnt = B <= BCAP;

  int64_t vt0 = blockIdx.x, vts = gridDim.x, vte = nvt;
  int mtb = (int)((int64_t)nrt * blockIdx.y / gridDim.y), mte = (int)((int64_t)nrt * (blockIdx.y + 1) / gridDim.y);
  if constexpr (MODE == TGT) {
    const int64_t b = blockIdx.x, t = a.target[b];
    const bool ok = t >= a.v_lo && t < a.v_hi;
    if (tid == 0) {
      a.rank[b] = ok ? 0 : -1;
      if (!ok) {
        a.ts[b] = 0.f;
        if (a.ts_out) a.ts_out[b] = 0.f;
      }
    }
    if (!ok) return;
    vt0 = (t - a.v_lo) / BV;
    vte = vt0 + 1;
    vts = 1;
    mtb = (int)(b / BR);
    mte = mtb + 1;
  }
  if (mte <= mtb) return;
  if constexpr (MODE == RANK) {
    if (lds_cnt)
      for (int i = tid; i < BCAP; i += NTH) accL[i] = 0;
  }

  const T* hp = reinterpret_cast<const T*>(a.h);
  const T* ep = reinterpret_cast<const T*>(a.E);

  // bf16, 16-B loadable E: the next vocabulary tile travels to registers under the last row tile's MFMAs and epilogue
  // (issued after that row tile's h loads: vmcnt retires in order) and is stored when the tile's readers are done.
  // Not in TOPK: with the 32 registers of the tile in flight its unrolled filter spills.
  constexpr bool PREF = !F32 && MODE != TOPK;
  u4 ex[8];
  auto e_load = [&](int64_t n0) {
    if constexpr (PREF) {
      const int cpr = a.dkp >> 3, nch = a.dkp >> 5;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int ch = tid + NTH * c, r = ch / cpr, k8 = (ch - r * cpr) * 8;
        ex[c] = (u4){0u, 0u, 0u, 0u};
        if (c < nch && n0 + r < a.v_hi && k8 < a.d) ex[c] = *reinterpret_cast<const u4*>(ep + (n0 + r) * a.lde + k8);
      }
    }
  };
  auto e_store = [&]() {
    if constexpr (PREF) {
      const int cpr = a.dkp >> 3, nch = a.dkp >> 5;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int ch = tid + NTH * c, r = ch / cpr, k8 = (ch - r * cpr) * 8;
        if (c < nch) *reinterpret_cast<u4*>(Et + r * P + k8) = ex[c];
      }
    }
  };
  if (PREF && a.vec_e) e_load(a.v_lo + vt0 * BV);

  for (int64_t vt = vt0; vt < vte; vt += vts) {
    const int64_t n0 = a.v_lo + vt * BV;
    float bia[FV][4];
#pragma unroll
    for (int i = 0; i < FV; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t v = n0 + v0w + 16 * i + 4 * g + r;
        bia[i][r] = (a.bias && v < a.v_hi) ? a.bias[v] : 0.f;
      }
    if constexpr (!F32) {
      __syncthreads();                       // the previous vocabulary tile's readers are done
      if (PREF && a.vec_e) e_store();
      else fill_tile(Et, ep, n0, a.v_hi, a.lde, a.vec_e, a.d, a.dkp, tid);
    }

    for (int mt = mtb; mt < mte; ++mt) {
      const int64_t m0 = (int64_t)mt * BR;
      __syncthreads();                       // the previous row tile's readers (Hs, mask, row metadata) are done
      // ---- row metadata, cleared mask, (bf16) the whole h tile
      if (tid < BR) {
        const int64_t row = m0 + tid;
        if constexpr (MODE == TOPK) {
          metaL[tid] = row < B ? ld_i32(a.cnt + (int64_t)blockIdx.x * B + row) : 0;
          thrL[tid] = row < B ? ld_u64(a.thr + (int64_t)blockIdx.x * B + row) : ~0ull;
          tsL[tid] = key_score(thrL[tid]);
        } else {
          int64_t t = row < B ? a.target[row] : -1;
          if (t < a.v_lo || t >= a.v_hi) t = -1;
          metaL[tid] = (int)t;
          if constexpr (MODE == RANK) tsL[tid] = (row < B && t >= 0) ? a.ts[row] : 0.f;
        }
      }
      if (has_ex) msk[tid] = 0u;             // NTH == BR * 4 words
      if constexpr (!F32) {
        fill_tile(Hs, hp, m0, B, a.ldh, a.vec_h, a.d, a.dkp, tid);
      }
      int cold = 0;                          // TOPK: some row of the tile has no threshold yet
      if constexpr (MODE == TOPK) cold = __syncthreads_or(tid < BR && m0 + tid < B && thrL[tid] == 0ull);
      else __syncthreads();
      if (PREF && a.vec_e && mt == mte - 1 && vt + vts < vte) e_load(a.v_lo + (vt + vts) * BV);
      // ---- exclusion bits of this (row tile, vocabulary tile): one thread per row, sorted list
      if (has_ex && tid < BR && m0 + tid < B) {
        const int64_t* p = a.excl + (m0 + tid) * a.ldx;
        int64_t lo = 0, hi = a.nx;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (p[mid] < n0) lo = mid + 1; else hi = mid;
        }
        for (; lo < a.nx; ++lo) {
          const int64_t off = p[lo] - n0;
          if (off >= BV) break;
          if (off < 0) continue;             // (an unsorted list: outside the contract, never outside the mask)
          msk[tid * 4 + (int)(off >> 5)] |= 1u << (int)(off & 31);
        }
      }

      // ---- S^T tile
      f32x4 acc[FV][4];
#pragma unroll
      for (int i = 0; i < FV; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (!F32) {
        for (int ks = 0; ks < a.dkp; ks += 32) {
          Frag<bf16> fa[FV], fb[4];
#pragma unroll
          for (int i = 0; i < FV; ++i) frag_load_vec(fa[i], Et + (v0w + 16 * i + cl) * P + ks + 8 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j) frag_load_vec(fb[j], Hs + (wn * 64 + 16 * j + cl) * P + ks + 8 * g);
#pragma unroll
          for (int i = 0; i < FV; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mma(fa[i], fb[j], acc[i][j]);
        }
      } else {
        const int r = tid >> 2, k8 = (tid & 3) * 8;
        const int64_t v = n0 + r, row = m0 + r;
        const float* erow = ep + (v < a.v_hi ? v : a.v_hi - 1) * a.lde;
        const float* hrow = hp + (row < B ? row : B - 1) * a.ldh;
        for (int ks = 0; ks < a.dkp; ks += FK) {
          float e8[8], h8[8];
          load8(e8, erow, ks + k8, a.d, a.vec_e, v < a.v_hi);
          load8(h8, hrow, ks + k8, a.d, a.vec_h, row < B);
          __syncthreads();                   // the previous chunk's fragments are read
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            Et[r * FP + k8 + e] = e8[e];
            Hs[r * FP + k8 + e] = h8[e];
          }
          __syncthreads();
          Frag<float> fa[FV], fb[4];
#pragma unroll
          for (int i = 0; i < FV; ++i) frag_load_vec(fa[i], Et + (v0w + 16 * i + cl) * FP + 8 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j) frag_load_vec(fb[j], Hs + (wn * 64 + 16 * j + cl) * FP + 8 * g);
#pragma unroll
          for (int i = 0; i < FV; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mma(fa[i], fb[j], acc[i][j]);
        }
      }
      __syncthreads();                       // the mask is complete
      // scores: + bias, -0 -> +0 (keys and float compares then agree)
#pragma unroll
      for (int i = 0; i < FV; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][r] = (acc[i][j][r] + bia[i][r]) + 0.0f;
      const int64_t vb = n0 + v0w + 4 * g;   // this lane's items: vb + 16 i + r

      if constexpr (MODE == TGT) {
        const int64_t b = blockIdx.x;
        const int rl = (int)(b - m0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (wn * 64 + 16 * j + cl == rl) {
            const int64_t t = metaL[rl];
#pragma unroll
            for (int i = 0; i < FV; ++i)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (vb + 16 * i + r == t) {
                  a.ts[b] = acc[i][j][r];
                  if (a.ts_out) a.ts_out[b] = acc[i][j][r];
                }
          }
      } else if constexpr (MODE == RANK) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rl = wn * 64 + 16 * j + cl;
          const int64_t t = metaL[rl];
          const float ts = tsL[rl];
          const unsigned mw = has_ex ? msk[rl * 4 + wm] : 0u;
          int c = 0;
#pragma unroll
          for (int i = 0; i < FV; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int64_t v = vb + 16 * i + r;
              const float s = acc[i][j][r];
              const bool ok = t >= 0 && v < a.v_hi && v != t && !((mw >> (16 * i + 4 * g + r)) & 1u);
              c += (ok && (s > ts || (s == ts && v < t))) ? 1 : 0;
            }
          c += __shfl_xor(c, 16, 64);
          c += __shfl_xor(c, 32, 64);
          if (g == 0 && c != 0) {
            if (lds_cnt) atomicAdd(accL + m0 + rl, c);
            else atomicAdd(a.rank + m0 + rl, c);
          }
        }
      } else {
        // pending candidates of this lane: bit 8 j + 4 i + r
        unsigned pend = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rl = wn * 64 + 16 * j + cl;
          const unsigned mw = has_ex ? msk[rl * 4 + wm] : 0u;
#pragma unroll
          for (int i = 0; i < FV; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool ok = m0 + rl < B && vb + 16 * i + r < a.v_hi && !((mw >> (16 * i + 4 * g + r)) & 1u);
              pend |= ok ? 1u << (8 * j + 4 * i + r) : 0u;
            }
        }
        // A tile that meets a row without a threshold would offer it all 128 items.  Its own bound first (K <= 16):
        // the K-th greatest of the 16 per-lane maxima of the row has K items at or above it, so anything below it
        // is not among the row's best K.  The scratch is the h tile, free since the MFMAs.
        float lb[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        if (cold && a.K <= 16) {
          float* mx = reinterpret_cast<float*>(Hs);            // [BR][16]
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float m = -__builtin_inff();
#pragma unroll
            for (int i = 0; i < FV; ++i)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (pend & (1u << (8 * j + 4 * i + r))) m = fmaxf(m, acc[i][j][r]);
            mx[(wn * 64 + 16 * j + cl) * 16 + wm * 4 + g] = m;
          }
          __syncthreads();
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (!((pend >> (8 * j)) & 0xffu)) continue;
            const float* x = mx + (wn * 64 + 16 * j + cl) * 16;
            for (int p = 0; p < 16; ++p) {
              const float xp = x[p];
              int rk = 0;
#pragma unroll
              for (int q = 0; q < 16; ++q) rk += (x[q] > xp || (x[q] == xp && q < p)) ? 1 : 0;
              if (rk == a.K - 1) lb[j] = xp;
            }
          }
        }
        const int cap = a.cap;
        bool filled = false;
        for (;;) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (!((pend >> (8 * j)) & 0xffu)) continue;
            const int rl = wn * 64 + 16 * j + cl;
            const u64 thr = thrL[rl];
            const float thrs = fmaxf(tsL[rl], lb[j]);   // one float compare drops nearly every candidate
            u64* list = a.lists + ((int64_t)blockIdx.x * B + m0 + rl) * cap;
#pragma unroll
            for (int i = 0; i < FV; ++i)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const unsigned bit = 1u << (8 * j + 4 * i + r);
                if (!(pend & bit)) continue;
                if (!(acc[i][j][r] >= thrs)) {
                  pend &= ~bit;
                  continue;
                }
                const u64 key = make_key(acc[i][j][r], (int)(vb + 16 * i + r));
                if (key <= thr) {
                  pend &= ~bit;              // at least K keys of this list are greater
                  continue;
                }
                const int pos = atomicAdd(metaL + rl, 1);
                filled |= pos >= cap - 1;
                if (pos < cap) {
                  st_u64(list + pos, key);
                  pend &= ~bit;
                }                            // else: no slot; again after the compaction below
              }
          }
          const int any = __syncthreads_or(pend != 0u || filled);   // (every slot taken above is written)
          if (!any) break;                   // the common round: nothing waits, no list is full
          // full lists (counts past cap: lanes that found no slot) -> their best K and a new threshold
          if (cap <= 64) {
            for (int r0 = wave; r0 < BR; r0 += 4 * (NTH / 64)) {
              u64* ls[4];
              int ns[4];
              u64 kth[4];
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const int rl = r0 + c * (NTH / 64);
                ns[c] = metaL[rl] >= cap ? cap : 0;
                ls[c] = a.lists + ((int64_t)blockIdx.x * B + m0 + rl) * cap;
              }
              if (ns[0] | ns[1] | ns[2] | ns[3]) {
                compact4(ls, ns, a.K, lane, kth);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                  if (ns[c] && lane == 0) {
                    const int rl = r0 + c * (NTH / 64);
                    metaL[rl] = a.K;
                    thrL[rl] = kth[c];
                    tsL[rl] = key_score(kth[c]);
                  }
              }
            }
          } else {
            for (int rl = wave; rl < BR; rl += NTH / 64) {
              if (metaL[rl] >= cap) {
                u64* list = a.lists + ((int64_t)blockIdx.x * B + m0 + rl) * cap;
                const u64 kth = compact(list, cap, a.K, lane);
                if (lane == 0) {
                  metaL[rl] = a.K;
                  thrL[rl] = kth;
                  tsL[rl] = key_score(kth);
                }
              }
            }
          }
          __syncthreads();
          filled = false;
        }
        if (tid < BR && m0 + tid < B) {
          st_i32(a.cnt + (int64_t)blockIdx.x * B + m0 + tid, metaL[tid]);
          st_u64(a.thr + (int64_t)blockIdx.x * B + m0 + tid, thrL[tid]);
        }
      }
    }
  }

  if constexpr (MODE == RANK) {
    if (lds_cnt) {
      __syncthreads();
      const int64_t r0 = (int64_t)mtb * BR, r1 = min(B, (int64_t)mte * BR);
      for (int64_t r = r0 + tid; r < r1; r += NTH)
        if (accL[r] != 0) atomicAdd(a.rank + r, accL[r]);
    }
  }
  if constexpr (MODE == TOPK) {
    // every list of this workgroup: its best K, sorted (the merge walks list heads)
    __syncthreads();
    const int64_t r0 = (int64_t)mtb * BR, r1 = min(B, (int64_t)mte * BR);
    if (a.cap <= 64) {
      for (int64_t rb = r0 + wave; rb < r1; rb += 4 * (NTH / 64)) {
        u64* ls[4];
        int ns[4];
        u64 kth[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int64_t r = rb + c * (NTH / 64);
          ns[c] = r < r1 ? ld_i32(a.cnt + (int64_t)blockIdx.x * B + r) : 0;
          ls[c] = a.lists + ((int64_t)blockIdx.x * B + r) * a.cap;
        }
        compact4(ls, ns, a.K, lane, kth);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (ns[c] > a.K && lane == 0) st_i32(a.cnt + (int64_t)blockIdx.x * B + rb + c * (NTH / 64), a.K);
      }
    } else {
      for (int64_t r = r0 + wave; r < r1; r += NTH / 64) {
        int* cp = a.cnt + (int64_t)blockIdx.x * B + r;
        const int n = ld_i32(cp);
        if (n > 0) {
          compact(a.lists + ((int64_t)blockIdx.x * B + r) * a.cap, n, a.K, lane);
          if (lane == 0) st_i32(cp, min(n, a.K));
        }
      }
    }
  }
}

// ids / scores of row b: K rounds of a block-wide max over the heads of the slices' sorted lists
__global__ __launch_bounds__(256) void merge_kernel(const u64* __restrict__ lists, const int* __restrict__ cnt, int nsl,
                                                    int64_t B, int K, int cap, int64_t* __restrict__ ids,
                                                    float* __restrict__ scores) {
  __shared__ u64 red[4];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const u64* list = lists + ((int64_t)tid * B + b) * cap;
  const int n = tid < nsl ? cnt[(int64_t)tid * B + b] : 0;
  int head = 0;
  u64 cur = n > 0 ? list[0] : 0ull;
  for (int r = 0; r < K; ++r) {
    const u64 w = wave_max64(cur);
    if ((tid & 63) == 0) red[tid >> 6] = w;
    __syncthreads();
    u64 best = red[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) best = red[q] > best ? red[q] : best;
    __syncthreads();
    if (tid == 0) {
      float s = -__builtin_inff();
      int64_t v = -1;
      if (best != 0ull) split_key(best, s, v);
      ids[b * K + r] = v;
      scores[b * K + r] = s;
    }
    if (best != 0ull && cur == best) {
      ++head;
      cur = head < n ? list[head] : 0ull;
    }
  }
}

// ---- rank -> Recall / NDCG / MRR @ k (one positive per row) -------------------------------------------------
constexpr int MAXK = 8;
__global__ __launch_bounds__(256) void rank_rows_kernel(const int* __restrict__ rank, int64_t R, int nk,
                                                        const int* __restrict__ ks, float* __restrict__ partial) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const int rk = rank[r];
  for (int q = 0; q < nk; ++q) {
    const bool hit = rk >= 0 && rk < ks[q];
    partial[r * 3 * nk + 3 * q + 0] = hit ? 1.f : 0.f;
    partial[r * 3 * nk + 3 * q + 1] = hit ? 1.f / log2f((float)rk + 2.f) : 0.f;
    partial[r * 3 * nk + 3 * q + 2] = hit ? 1.f / ((float)rk + 1.f) : 0.f;
  }
}
// mean over rows in double, fixed order (one workgroup) -- sampler.hip's rank_mean_kernel
__global__ __launch_bounds__(256) void mean_kernel(const float* __restrict__ partial, int64_t R, int m,
                                                   float* __restrict__ out) {
  __shared__ double red[256];
  for (int c = 0; c < m; ++c) {
    double acc = 0.0;
    for (int64_t r = threadIdx.x; r < R; r += 256) acc += (double)partial[r * m + c];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = (float)(red[0] / (double)R);
    __syncthreads();
  }
}

template <typename T, int MODE>
hipError_t launch(const Args& a, dim3 grid, hipStream_t s) {
  const int lds = lds_bytes<T, MODE>(a.dkp);
  static int attr = 0;
  if (attr < lds) {
    (void)hipFuncSetAttribute((const void*)sweep_kernel<T, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr = lds;
  }
  hipLaunchKernelGGL((sweep_kernel<T, MODE>), grid, dim3(NTH), lds, s, a);
  return hipGetLastError();
}

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
inline int64_t slices_of(int64_t nrange) { return std::min<int64_t>(cdiv(nrange, BV), NSL); }
// workspace: target scores [B] | thr [nsl][B] | cnt [nsl][B] | lists [nsl][B][cap]
inline int64_t ts_bytes(int64_t B) { return align256(B * 4); }
inline int64_t state_bytes(int64_t nsl, int64_t B) { return align256(nsl * B * 8) + align256(nsl * B * 4); }

int check(int dtype, const void* h, int64_t ldh, int64_t B, int64_t d, const void* E, int64_t lde, int64_t v_lo,
          int64_t v_hi, const int64_t* excl, int64_t nx, int64_t ldx, const void* ws) {
  if ((dtype != RS_DTYPE_F32 && dtype != RS_DTYPE_BF16) || !h || !E || !ws || B <= 0 || d <= 0 || ldh < d || lde < d ||
      v_lo < 0 || v_hi <= v_lo || nx < 0 || (excl && nx > 0 && ldx < nx))
    return RS_ERR_ARG;
  if (d > 256 || v_hi > 0x7fffff00ll || B > 0x7fffff00ll) return RS_ERR_UNSUPPORTED;
  return RS_OK;
}

Args make_args(int dtype, const void* h, int64_t ldh, int64_t B, int64_t d, const void* E, int64_t lde,
               const float* bias, int64_t v_lo, int64_t v_hi, const int64_t* excl, int64_t nx, int64_t ldx) {
  Args a = {};
  const int64_t el = dtype == RS_DTYPE_F32 ? 4 : 2, per = 16 / el;
  a.h = h; a.ldh = ldh; a.E = E; a.lde = lde; a.bias = bias;
  a.B = B; a.d = (int)d; a.dkp = (int)((d + 31) / 32 * 32);
  a.v_lo = v_lo; a.v_hi = v_hi;
  a.excl = nx > 0 ? excl : nullptr; a.nx = nx; a.ldx = ldx;
  a.vec_h = d % 8 == 0 && ldh % per == 0 && (uintptr_t)h % 16 == 0;
  a.vec_e = d % 8 == 0 && lde % per == 0 && (uintptr_t)E % 16 == 0;
  return a;
}

dim3 sweep_grid(int64_t B, int64_t nrange) {
  const int64_t gx = slices_of(nrange), nrt = cdiv(B, BR);
  // fewer vocabulary tiles than CUs: split the row tiles over gridDim.y groups (each (row, item) still once)
  const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(nrt, NSL / gx));
  return dim3((unsigned)gx, (unsigned)gy);
}
}  // namespace fr

extern "C" {

int64_t rs_full_ws_bytes(int dtype, int64_t B, int64_t d, int64_t nrange, int64_t K) {
  (void)dtype; (void)d;
  if (B <= 0 || nrange <= 0 || K < 0 || K > RS_TOPK_MAX) return 0;
  int64_t n = fr::ts_bytes(B);
  if (K > 0) {
    const int64_t nsl = fr::slices_of(nrange);
    n += fr::state_bytes(nsl, B) + nsl * B * fr::cap_of((int)K) * 8;
  }
  return n;
}

int rs_full_rank(int dtype, const void* h, int64_t ldh, int64_t B, int64_t d, const void* E, int64_t lde,
                 const float* bias, int64_t v_lo, int64_t v_hi, const int64_t* target, const int64_t* excl, int64_t nx,
                 int64_t ldx, void* ws, int* rank, float* target_score, void* stream) {
  const int rc = fr::check(dtype, h, ldh, B, d, E, lde, v_lo, v_hi, excl, nx, ldx, ws);
  if (rc != RS_OK) return rc;
  if (!target || !rank) return RS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  fr::Args a = fr::make_args(dtype, h, ldh, B, d, E, lde, bias, v_lo, v_hi, excl, nx, ldx);
  a.target = target; a.rank = rank; a.ts = (float*)ws; a.ts_out = target_score;
  const dim3 g = fr::sweep_grid(B, v_hi - v_lo);
  hipError_t e;
  if (dtype == RS_DTYPE_F32) {
    e = fr::launch<float, fr::TGT>(a, dim3((unsigned)B), s);
    if (e == hipSuccess) e = fr::launch<float, fr::RANK>(a, g, s);
  } else {
    e = fr::launch<__bf16, fr::TGT>(a, dim3((unsigned)B), s);
    if (e == hipSuccess) e = fr::launch<__bf16, fr::RANK>(a, g, s);
  }
  return (int)e;
}

int rs_full_topk(int dtype, const void* h, int64_t ldh, int64_t B, int64_t d, const void* E, int64_t lde,
                 const float* bias, int64_t v_lo, int64_t v_hi, const int64_t* excl, int64_t nx, int64_t ldx, int64_t K,
                 void* ws, int64_t* ids, float* scores, void* stream) {
  const int rc = fr::check(dtype, h, ldh, B, d, E, lde, v_lo, v_hi, excl, nx, ldx, ws);
  if (rc != RS_OK) return rc;
  if (!ids || !scores || K < 1) return RS_ERR_ARG;
  if (K > RS_TOPK_MAX) return RS_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  fr::Args a = fr::make_args(dtype, h, ldh, B, d, E, lde, bias, v_lo, v_hi, excl, nx, ldx);
  const int64_t nsl = fr::slices_of(v_hi - v_lo);
  char* p = (char*)ws + fr::ts_bytes(B);
  a.thr = (fr::u64*)p;
  a.cnt = (int*)(p + fr::align256(nsl * B * 8));
  a.lists = (fr::u64*)(p + fr::state_bytes(nsl, B));
  a.K = (int)K; a.cap = fr::cap_of((int)K);
  if (hipMemsetAsync(p, 0, (size_t)fr::state_bytes(nsl, B), s) != hipSuccess) return (int)hipGetLastError();
  const dim3 g = fr::sweep_grid(B, v_hi - v_lo);
  hipError_t e = dtype == RS_DTYPE_F32 ? fr::launch<float, fr::TOPK>(a, g, s) : fr::launch<__bf16, fr::TOPK>(a, g, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(fr::merge_kernel, dim3((unsigned)B), dim3(256), 0, s, a.lists, a.cnt, (int)nsl, B, (int)K, a.cap,
                     ids, scores);
  return (int)hipGetLastError();
}

int rs_rank_to_metrics(const int* rank, int64_t rows, int nk, const int* ks, float* ws, float* out, void* stream) {
  if (!rank || rows <= 0 || nk <= 0 || nk > fr::MAXK || !ks || !ws || !out) return RS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fr::rank_rows_kernel, dim3((unsigned)cdiv(rows, 256)), dim3(256), 0, s, rank, rows, nk, ks, ws);
  hipLaunchKernelGGL(fr::mean_kernel, dim3(1), dim3(256), 0, s, ws, rows, 3 * nk, out);
  return (int)hipGetLastError();
}

}  // extern "C"
