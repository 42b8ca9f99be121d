// Sampled-softmax head of SASRec over batch-shared candidates (gfx950).
//
// The objective, on the compact valid rows rs_sas_ce_rows_fwd leaves (hl [cap][d], lab [cap], *count):
//   f_r   = last_layernorm(log2feats(seq))[r]          for every position r with pos_r != 0 ("valid")
//   z_r0  = <f_r, E[pos_r]>                            E = item_emb.weight (tied), fp32 accumulate
//   z_rj  = <f_r, E[cand_j]>,  j = 1..K                cand: int64 [K], ids in [0, V]
//   live(r, j) = cand_j != 0 and cand_j != pos_r       id 0 = an ignored slot; accidental hits masked
//   loss  = (1 / max(n, 1)) * sum_valid r [ log( exp(z_r0) + sum_{live j} exp(z_rj) ) - z_r0 ],   n = #valid
// Duplicate candidates are separate classes; the logQ correction is the rs_sce_head_logq_* entries' (below); a row
// without a live candidate has loss 0 and gradient 0; with cand = 1..V it is the full-catalogue cross-entropy up to
// the padding class 0 (logit exactly 0),
// which the full loss counts and a candidate list cannot name.  Gradients, with p = softmax over {0} + live:
// d f_r = ((p_r0 - 1) E[pos_r] + sum_live p_rj E[cand_j]) / n;  the table gets (p_r0 - 1) / n * f_r at row pos_r and
// sum_r p_rj / n * f_r at row cand_j.
//
// One sweep kernel, three roles.  A workgroup (4 waves) owns 64 STATIONARY items, 16 per wave, as MFMA B fragments
// in registers, and sweeps the other side in LDS tiles of 64 items (rows gathered by id straight from the table):
//   forward   stationary = rows of hl, swept = the K candidates: z tile = W S^T (v_mfma_f32_16x16x32_bf16 / the exact
//             fp32 MFMA), a masked online max / sum per row; each lane carries its own (m, s) over the candidates its
//             accumulator rows cover and the four are merged once at the end.  The candidate tiles are split over
//             blockIdx.y (rs_sas_sce_dh_splits: the sweep is a chain of dependent tile loads, and 64 rows per
//             workgroup alone leave most of the device idle); each split leaves its (m, s) per row and a small second
//             launch merges them in split order -- no atomics, no fence.  The positive's logit is a plain fp32 dot.
//   dh        the same sweep; p = exp(z - lse) of the live pairs goes back into the MFMA as the A operand
//             (dh = P Ec), the accumulator's 4 swept items of two 16-item sub-tiles filling one 8-deep k group.  Each
//             candidate split writes its own fp32 slab [cap][d]: rs_sas_ce_rows_bwd sums them in split order.
//   dEc       the roles swapped: stationary = 64 candidates, swept = a split of the rows; dEc = P^T hl.  The row
//             splits go to fp32 slabs reduced in split order (launch_reduce_slabs): a fixed summation order, no
//             atomics.
// The logits are never stored.  Widths: d <= 128 (padded with zeros to 64 or 128 in the fragments), fp32 or bf16
// (bf16: d % 8 == 0); d in {64, 128} with aligned rows loads 16 bytes at a time.  128 < d <= 1024: generic_kernel,
// the same sweep with plain FMA (below).
//
// The rs_sce_head_* entries run the same kernels for an untied output layer E [V1][d] with a bias b [V1] (BERT4Rec's
// out.weight / out.bias): z_r0 = <h_r, E[lab_r]> + b[lab_r], z_rj = <h_r, E[cand_j]> + b[cand_j]; everything else is
// computed on these logits as above, and the dEc role also leaves dbc[j] = s sum_r p_rj (each lane's live p summed
// over its swept rows in sweep order, the four lane groups by two shuffles, the row splits through slabs reduced in
// split order: no atomics).  The bias gradient at the positive is coef[r].  They also take bf16 128 < d <= 256 on the
// MFMA sweep (DP = 256: 8 stationary fragments, 16 accumulators per lane, a 33 KB LDS tile); fp32 would need a 67 KB
// tile and stays on generic_kernel past 128.  Without a bias they give the rs_sas_sce_* entries' bits wherever both run
// the same kernel.
//
// The rs_sce_head_logq_* entries subtract logq[id], the log of the proposal the candidates were drawn from (fp32 [V1],
// not a parameter): every logit takes the one per-id term b[id] - logq[id] where it took b[id] -- the swept ids' term
// staged in LDS (forward, dh), the stationary candidate's (dEc), the positive's z0.  The tile loop is the biased
// head's, and logq == NULL leaves the bits of the entries above.  rs_alias_items draws the candidates from that proposal.
#include "common.h"
#include "../../include/recsys_hip.h"

namespace sce {

constexpr int TS = 64;             // items per stationary set and per swept LDS tile
constexpr int64_t KMAX = 65536;    // most candidates (RS_SAS_SCE_MAX_K)
constexpr int MAX_SPLITS = 64;     // most row splits of the dEc launch
constexpr float NEG = -3.0e38f;    // "no live logit yet" (finite: NEG - NEG = 0, expf(NEG - z) = 0)

enum { FWD = 0, DH = 1, DEC = 2 };

struct Args {
  const void* hl;
  int64_t ldh;
  const int64_t* lab;
  const int32_t* cnt;
  int64_t cap;
  const void* E;
  int64_t V1;
  const int64_t* cand;
  int64_t K;
  int d, vec;
  float* lse;
  float* z0;
  float* pm;       // forward: the candidate splits' partial (max, sum) per row, [ksplits][cap] each
  float* ps;
  const float* div;
  const float* dloss;
  float* dh;
  float* coef;
  float* pg;
  float* slab;
  int64_t rows_per_split;
  const float* bias;   // [V1] or null: added to every logit (rs_sce_head_*)
  float* dbslab;       // dEc role: sum over the split's rows of p per candidate, [splits][K]; null without a bias
  const float* logq;   // [V1] or null: subtracted from every logit (rs_sce_head_logq_*); not a parameter, no gradient
};

// the per-id additive term of a logit: bias[id] - logq[id] in fp32 (either may be absent; id != 0, so logq[0] is
// never read).  With logq null it is bias[id], the bits of the entries without a correction.
__device__ __forceinline__ float id_term(const Args& a, int32_t id) {
  const float b = a.bias ? a.bias[id] : 0.f;
  return a.logq ? b - a.logq[id] : b;
}

__device__ __forceinline__ int32_t clamp_id(int64_t v, int64_t V1) { return (v <= 0 || v >= V1) ? 0 : (int32_t)v; }

// elements k0 .. k0 + 7 of a row of width d as a fragment (zeros past d or for a null row)
template <typename T>
__device__ __forceinline__ void load8(Frag<T>& f, const T* row, int k0, int d, bool vec) {
  if (!row || k0 >= d) {
    frag_zero(f);
    return;
  }
  if (vec && k0 + 8 <= d) {
    frag_load_vec(f, row + k0);
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) frag_set(f, j, k0 + j < d ? to_f(row[k0 + j]) : 0.f);
}

__device__ __forceinline__ void lds_store8(__bf16* p, const Frag<__bf16>& f) { *reinterpret_cast<bf16x8*>(p) = f.v; }
__device__ __forceinline__ void lds_store8(float* p, const Frag<float>& f) {
  *reinterpret_cast<float4*>(p) = make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(f.v[4], f.v[5], f.v[6], f.v[7]);
}

template <typename T, int DP, int MODE>
__global__ __launch_bounds__(256) void sweep_kernel(Args a) {
  constexpr int LDW = DP + 8, KK = DP / 32, NT = DP / 16, CPR = DP / 8;
  __shared__ __attribute__((aligned(16))) T W[TS * LDW];
  __shared__ int32_t sWid[TS];
  __shared__ float sWlse[TS];
  __shared__ int32_t sSid[TS];
  __shared__ float sScoef[TS];
  __shared__ float sWb[TS];                           // the swept candidates' bias - logq (forward, dh)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int d = a.d;
  const bool vec = a.vec != 0;
  const bool term = a.bias || a.logq;                 // a per-id term joins the logits
  const int64_t count = a.cnt ? min((int64_t)*a.cnt, a.cap) : a.cap;
  const T* HL = (const T*)a.hl;
  const T* E = (const T*)a.E;
  const int64_t s0 = (int64_t)blockIdx.x * TS;
  if (MODE != DEC && s0 >= count) return;          // the whole workgroup: no barrier is left waiting

  auto row_id = [&](int64_t r) -> int32_t { return r < count ? clamp_id(a.lab[r], a.V1) : 0; };
  auto cand_id = [&](int64_t j) -> int32_t { return j < a.K ? clamp_id(a.cand[j], a.V1) : 0; };

  // this lane's stationary item (c of the wave's 16): id, row, fragments S[kk] = item[kk * 32 + 8 g .. + 7]
  const int64_t si = s0 + wave * 16 + c;
  const int32_t sid = MODE == DEC ? cand_id(si) : row_id(si);
  const T* srow = !sid ? nullptr : (MODE == DEC ? E + (int64_t)sid * d : HL + si * a.ldh);
  Frag<T> S[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) load8(S[kk], srow, kk * 32 + 8 * g, d, vec);
  float slse = 0.f, z0 = 0.f;
  if (MODE == FWD) {
    const T* prow = sid ? E + (int64_t)sid * d : nullptr;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      Frag<T> P;
      load8(P, prow, kk * 32 + 8 * g, d, vec);
#pragma unroll
      for (int j = 0; j < 8; ++j) z0 = __builtin_fmaf(to_f(S[kk].v[j]), to_f(P.v[j]), z0);
    }
    z0 += __shfl_xor(z0, 16, 64);
    z0 += __shfl_xor(z0, 32, 64);
    if (term && sid) z0 += id_term(a, sid);
  } else if (MODE == DH && sid) {
    slse = a.lse[si];
    z0 = a.z0[si];
  }

  // the swept range of this workgroup: blockIdx.y = a split of the rows (dEc) or of the candidate tiles (forward, dh)
  int64_t w_begin, w_end;
  if (MODE == DEC) {
    w_begin = (int64_t)blockIdx.y * a.rows_per_split;
    w_end = min(count, w_begin + a.rows_per_split);
  } else {
    const int64_t per = cdiv(cdiv(a.K, (int64_t)TS), (int64_t)gridDim.y) * TS;
    w_begin = (int64_t)blockIdx.y * per;
    w_end = min(a.K, w_begin + per);
  }
  // ids of the next tile's rows, one per 16-byte chunk this thread copies: loaded a tile ahead, so that a tile's
  // row loads do not wait for its id loads
  constexpr int NCH = TS * CPR / 256;
  int32_t nid[NCH];
  auto tile_ids = [&](int64_t w0) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int64_t wi = w0 + (tid + i * 256) / CPR;
      nid[i] = wi < w_end ? (MODE == DEC ? row_id(wi) : cand_id(wi)) : 0;
    }
  };
  if (w_begin < w_end) tile_ids(w_begin);
  float m = NEG, s = 0.f;
  // dEc: the stationary candidate's bias - logq, and (with a bias) this lane's sum of p over the rows it met
  const float sbias = MODE == DEC && term && sid ? id_term(a, sid) : 0.f;
  float psum = 0.f;
  f32x4 O[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) O[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t w0 = w_begin; w0 < w_end; w0 += TS) {
    __syncthreads();                                  // the previous tile has been consumed
    if (tid < TS) {
      const int64_t wi = w0 + tid;
      int32_t id = 0;
      float l = 0.f;
      if (wi < w_end) {
        if (MODE == DEC) {
          id = row_id(wi);
          if (id) l = a.lse[wi];
        } else {
          id = cand_id(wi);
        }
      }
      sWid[tid] = id;
      sWlse[tid] = l;
      if (MODE != DEC && term) sWb[tid] = id ? id_term(a, id) : 0.f;
    }
    Frag<T> fr[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * 256, e = ch / CPR, k0 = (ch % CPR) * 8;
      const T* row = !nid[i] ? nullptr : (MODE == DEC ? HL + (w0 + e) * a.ldh : E + (int64_t)nid[i] * d);
      load8(fr[i], row, k0, d, vec);
    }
    if (w0 + TS < w_end) tile_ids(w0 + TS);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * 256;
      lds_store8(&W[(ch / CPR) * LDW + (ch % CPR) * 8], fr[i]);
    }
    __syncthreads();
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {                  // two 16-item sub-tiles = one 32-deep k chunk of P
      Frag<T> Pf;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int sub = sp * 2 + h;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          Frag<T> A;
          frag_load_vec(A, &W[(sub * 16 + c) * LDW + kk * 32 + 8 * g]);
          acc = mma(A, S[kk], acc);                   // acc[r] = z[swept sub * 16 + 4 g + r][stationary c]
        }
        if (term) {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] += MODE == DEC ? sbias : sWb[sub * 16 + 4 * g + r];
        }
        bool lv[4];
        float zm = NEG;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int wi = sub * 16 + 4 * g + r;
          const int32_t wid = sWid[wi];
          const int32_t cid = MODE == DEC ? sid : wid, rid = MODE == DEC ? wid : sid;
          lv[r] = cid != 0 && rid != 0 && cid != rid;
          if (MODE == FWD) {
            if (lv[r]) zm = fmaxf(zm, acc[r]);
          } else {
            const float l = MODE == DEC ? sWlse[wi] : slse;
            const float p = lv[r] ? expf(acc[r] - l) : 0.f;
            frag_set(Pf, h * 4 + r, p);
            if (MODE == DEC) psum += p;
          }
        }
        if (MODE == FWD && zm > NEG) {
          const float mn = fmaxf(m, zm);
          float t = 0.f;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (lv[r]) t += expf(acc[r] - mn);
          s = s * expf(m - mn) + t;
          m = mn;
        }
      }
      if (MODE != FWD) {
        // out[stationary][col] += sum over the 32 swept items of p * W[item][col]; k slot 8 g + j holds item
        // sp * 32 + 4 g + j (j < 4) or sp * 32 + 16 + 4 g + j - 4: the order the accumulators left p in
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          Frag<T> B;
#pragma unroll
          for (int j = 0; j < 8; ++j) B.v[j] = W[(sp * 32 + (j >> 2) * 16 + 4 * g + (j & 3)) * LDW + nt * 16 + c];
          O[nt] = mma(Pf, B, O[nt]);                  // O[nt][r] = out[stationary 4 g + r][col nt * 16 + c]
        }
      }
    }
  }

  if (MODE == FWD) {
    // merge the four lane groups' (m, s) of row c: a symmetric pairwise step, so every lane ends with the same bits
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float mo = __shfl_xor(m, o, 64), so = __shfl_xor(s, o, 64);
      const float mn = fmaxf(m, mo);
      s = s * expf(m - mn) + so * expf(mo - mn);
      m = mn;
    }
    if (g == 0 && si < count) {                       // this split's part of the row's sum; combine_kernel merges them
      a.pm[(int64_t)blockIdx.y * a.cap + si] = m;
      a.ps[(int64_t)blockIdx.y * a.cap + si] = s;
      if (blockIdx.y == 0) a.z0[si] = sid ? z0 : 0.f;
    }
    return;
  }
  const float scale = (a.dloss ? *a.dloss : 1.f) / *a.div;
  if (MODE == DH) {
    // the positive's term and the per-row outputs: the first candidate split's
    const float cf = sid && blockIdx.y == 0 ? (expf(z0 - slse) - 1.f) * scale : 0.f;
    if (g == 0) {
      sSid[wave * 16 + c] = sid;
      sScoef[wave * 16 + c] = cf;
      if (si < count && blockIdx.y == 0) a.coef[si] = cf;
    }
    float* dh = a.dh + (int64_t)blockIdx.y * a.cap * d;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int li = wave * 16 + 4 * g + r;
      const int64_t row = s0 + li;
      if (row >= count) continue;
      const int32_t id = sSid[li];
      const float cr = sScoef[li];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int col = nt * 16 + c;
        if (col >= d) continue;
        if (blockIdx.y != 0) {
          dh[row * d + col] = scale * O[nt][r];
          continue;
        }
        const float e = id ? to_f(E[(int64_t)id * d + col]) : 0.f;
        const float h = id ? to_f(HL[row * a.ldh + col]) : 0.f;
        dh[row * d + col] = scale * O[nt][r] + cr * e;
        a.pg[row * d + col] = cr * h;
      }
    }
    return;
  }
  if (a.dbslab) {                                     // uniform: the four lane groups' sums of candidate c, in order
    psum += __shfl_xor(psum, 16, 64);
    psum += __shfl_xor(psum, 32, 64);
    const int64_t j = s0 + wave * 16 + c;
    if (g == 0 && j < a.K) a.dbslab[(int64_t)blockIdx.y * a.K + j] = scale * psum;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t j = s0 + wave * 16 + 4 * g + r;
    if (j >= a.K) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = nt * 16 + c;
      if (col < d) a.slab[((int64_t)blockIdx.y * a.K + j) * d + col] = scale * O[nt][r];
    }
  }
}

// The generic form of the same sweep for 128 < d <= GEN_DMAX (fp32, or bf16 with d % 8 == 0): plain FMA, no LDS
// tile.  One workgroup per stationary item, its vector spread over a wave's lanes (element k in lane k % 64), held by
// each of the 4 waves; wave w takes the live swept items w, w + 4, ... of the workgroup's range, a wave-wide dot
// product each.  The waves' (m, s) / output rows are merged through LDS in wave order: a fixed order, no atomics.
// Same splits over blockIdx.y, same outputs as sweep_kernel.  Slow, and meant to be: the widths the fused blocks
// do not cover either.
constexpr int GEN_DMAX = 1024, GEN_C = GEN_DMAX / 64;

template <typename T, int MODE>
__global__ __launch_bounds__(256) void generic_kernel(Args a) {
  __shared__ float red[4 * GEN_DMAX];
  __shared__ float rm[4], rs[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = a.d;
  const int64_t count = a.cnt ? min((int64_t)*a.cnt, a.cap) : a.cap;
  const T* HL = (const T*)a.hl;
  const T* E = (const T*)a.E;
  const int64_t si = blockIdx.x;
  if (MODE != DEC && si >= count) return;
  auto row_id = [&](int64_t r) -> int32_t { return r < count ? clamp_id(a.lab[r], a.V1) : 0; };
  auto cand_id = [&](int64_t j) -> int32_t { return j < a.K ? clamp_id(a.cand[j], a.V1) : 0; };
  const int32_t sid = MODE == DEC ? cand_id(si) : row_id(si);
  const T* srow = !sid ? nullptr : (MODE == DEC ? E + (int64_t)sid * d : HL + si * a.ldh);
  float sv[GEN_C], acc[GEN_C];
#pragma unroll
  for (int i = 0; i < GEN_C; ++i) {
    const int k = lane + 64 * i;
    sv[i] = srow && k < d ? to_f(srow[k]) : 0.f;
    acc[i] = 0.f;
  }
  float slse = 0.f, z0 = 0.f;
  if (MODE == FWD && sid) {
    const T* prow = E + (int64_t)sid * d;
#pragma unroll
    for (int i = 0; i < GEN_C; ++i) {
      const int k = lane + 64 * i;
      if (k < d) z0 = __builtin_fmaf(sv[i], to_f(prow[k]), z0);
    }
    z0 = wave_sum(z0);
    if (a.bias || a.logq) z0 += id_term(a, sid);
  } else if (MODE == DH && sid) {
    slse = a.lse[si];
    z0 = a.z0[si];
  }
  int64_t w_begin, w_end;
  if (MODE == DEC) {
    w_begin = (int64_t)blockIdx.y * a.rows_per_split;
    w_end = min(count, w_begin + a.rows_per_split);
  } else {
    const int64_t per = cdiv(cdiv(a.K, (int64_t)TS), (int64_t)gridDim.y) * TS;
    w_begin = (int64_t)blockIdx.y * per;
    w_end = min(a.K, w_begin + per);
  }
  float m = NEG, s = 0.f, psum = 0.f;
  for (int64_t wi = w_begin + wave; wi < w_end; wi += 4) {
    const int32_t wid = MODE == DEC ? row_id(wi) : cand_id(wi);
    const int32_t cid = MODE == DEC ? sid : wid, rid = MODE == DEC ? wid : sid;
    if (cid == 0 || rid == 0 || cid == rid) continue;            // not live (the whole wave)
    const T* wrow = MODE == DEC ? HL + wi * a.ldh : E + (int64_t)wid * d;
    float wv[GEN_C], z = 0.f;
#pragma unroll
    for (int i = 0; i < GEN_C; ++i) {
      const int k = lane + 64 * i;
      wv[i] = k < d ? to_f(wrow[k]) : 0.f;
      z = __builtin_fmaf(sv[i], wv[i], z);
    }
    z = wave_sum(z);
    if (a.bias || a.logq) z += id_term(a, cid);
    if (MODE == FWD) {
      const float mn = fmaxf(m, z);
      s = s * expf(m - mn) + expf(z - mn);
      m = mn;
    } else {
      const float p = expf(z - (MODE == DEC ? a.lse[wi] : slse));
      psum += p;
#pragma unroll
      for (int i = 0; i < GEN_C; ++i) acc[i] = __builtin_fmaf(p, wv[i], acc[i]);
    }
  }
  if (MODE == FWD) {
    if (lane == 0) {
      rm[wave] = m;
      rs[wave] = s;
    }
    __syncthreads();
    if (tid == 0) {
      m = rm[0];
      s = rs[0];
      for (int w = 1; w < 4; ++w) {
        const float mn = fmaxf(m, rm[w]);
        s = s * expf(m - mn) + rs[w] * expf(rm[w] - mn);
        m = mn;
      }
      a.pm[(int64_t)blockIdx.y * a.cap + si] = m;
      a.ps[(int64_t)blockIdx.y * a.cap + si] = s;
      if (blockIdx.y == 0) a.z0[si] = sid ? z0 : 0.f;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < GEN_C; ++i) {
    const int k = lane + 64 * i;
    if (k < d) red[wave * d + k] = acc[i];
  }
  if (lane == 0) rm[wave] = psum;
  __syncthreads();
  const float scale = (a.dloss ? *a.dloss : 1.f) / *a.div;
  const bool first = blockIdx.y == 0;
  if (MODE == DEC && a.dbslab && tid == 0)
    a.dbslab[(int64_t)blockIdx.y * a.K + si] = scale * (((rm[0] + rm[1]) + rm[2]) + rm[3]);
  const float cf = MODE == DH && sid && first ? (expf(z0 - slse) - 1.f) * scale : 0.f;
  if (MODE == DH && first && tid == 0) a.coef[si] = cf;
  for (int col = tid; col < d; col += 256) {
    const float t = ((red[col] + red[d + col]) + red[2 * d + col]) + red[3 * d + col];
    if (MODE == DEC) {
      a.slab[((int64_t)blockIdx.y * a.K + si) * d + col] = scale * t;
    } else if (!first) {
      a.dh[((int64_t)blockIdx.y * a.cap + si) * d + col] = scale * t;
    } else {
      const float e = sid ? to_f(E[(int64_t)sid * d + col]) : 0.f;
      const float h = sid ? to_f(HL[si * a.ldh + col]) : 0.f;
      a.dh[si * d + col] = scale * t + cf * e;
      a.pg[si * d + col] = cf * h;
    }
  }
}

// lse per row from the candidate splits' (max, sum), merged in split order, and the positive's logit; the loss terms
// lse - z0 of the block's 256 rows summed in double, in a fixed order: part[block] = {sum, valid rows}
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ pm, const float* __restrict__ ps, int ks,
                                                      const int64_t* __restrict__ lab, const int32_t* cnt, int64_t cap,
                                                      int64_t V1, const float* __restrict__ z0, float* __restrict__ lse,
                                                      double* __restrict__ part) {
  __shared__ double red[256];
  __shared__ int nred[256];
  const int64_t count = cnt ? min((int64_t)*cnt, cap) : cap;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double loss = 0.0;
  int n = 0;
  if (r < count) {
    float l = 0.f;
    if (clamp_id(lab[r], V1)) {
      float m = pm[r], s = ps[r];
      for (int y = 1; y < ks; ++y) {
        const float mo = pm[(int64_t)y * cap + r], so = ps[(int64_t)y * cap + r];
        const float mn = fmaxf(m, mo);
        s = s * expf(m - mn) + so * expf(mo - mn);
        m = mn;
      }
      const float z = z0[r], M = fmaxf(m, z);
      l = M + logf(expf(z - M) + s * expf(m - M));
      loss = (double)l - (double)z;
      n = 1;
    }
    lse[r] = l;
  }
  red[threadIdx.x] = loss;
  nred[threadIdx.x] = n;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      red[threadIdx.x] += red[threadIdx.x + st];
      nred[threadIdx.x] += nred[threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = red[0];
    part[2 * blockIdx.x + 1] = (double)nred[0];
  }
}

// out = {sum of the blocks' loss sums, number of valid rows, sum / *div}: one workgroup, a fixed order
__global__ __launch_bounds__(256) void finish_kernel(const double* __restrict__ part, int64_t nb, const float* div,
                                                     float* __restrict__ out) {
  __shared__ double red[256], nred[256];
  double acc = 0.0, n = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += 256) {
    acc += part[2 * b];
    n += part[2 * b + 1];
  }
  red[threadIdx.x] = acc;
  nred[threadIdx.x] = n;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      red[threadIdx.x] += red[threadIdx.x + st];
      nred[threadIdx.x] += nred[threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)red[0];
    out[1] = (float)nred[0];
    out[2] = (float)(red[0] / (double)*div);
  }
}

// keys of the table gradient's inverted index: the positives of the rows < count, then the candidates (0 = no row)
__global__ __launch_bounds__(256) void keys_kernel(const int64_t* __restrict__ lab, const int32_t* cnt, int64_t cap,
                                                   const int64_t* __restrict__ cand, int64_t K, int64_t V1,
                                                   int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap + K) return;
  const int64_t count = cnt ? min((int64_t)*cnt, cap) : cap;
  keys[i] = i < cap ? (i < count ? clamp_id(lab[i], V1) : 0) : clamp_id(cand[i - cap], V1);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void uniform_items_kernel(const uint64_t* seed_base, uint64_t salt, int64_t item_num,
                                                            int64_t K, int64_t* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  const uint64_t seed = eff_seed(salt, seed_base);
  out[j] = 1 + (int64_t)__umul64hi(splitmix64(seed + 0x632BE59BD9B4E019ull * (uint64_t)(j + 1)), (uint64_t)item_num);
}

// One draw from the packed alias table (entry s = thr[s] | (uint64_t)alias[s] << 32): the high word of r * V picks
// the slot, the next 32 bits decide between the slot's own item and its alias.
__global__ __launch_bounds__(256) void alias_items_kernel(const uint64_t* seed_base, uint64_t salt,
                                                          const uint64_t* __restrict__ table, int64_t item_num,
                                                          int64_t K, int64_t* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  const uint64_t seed = eff_seed(salt, seed_base);
  const uint64_t r = splitmix64(seed + 0x632BE59BD9B4E019ull * (uint64_t)(j + 1));
  const uint64_t slot = __umul64hi(r, (uint64_t)item_num);          // < item_num
  const uint32_t frac = (uint32_t)((r * (uint64_t)item_num) >> 32);
  const uint64_t e = table[slot];
  out[j] = frac < (uint32_t)e ? (int64_t)slot + 1 : (int64_t)(e >> 32);
}

static int splits_of(int64_t cap, int64_t K, int64_t* rows_per_split) {
  const int64_t nct = cdiv(K, (int64_t)TS), tiles = cdiv(cap, (int64_t)TS);
  int64_t sp = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(MAX_SPLITS, tiles), cdiv(512, nct)));
  const int64_t rps = cdiv(tiles, sp) * TS;
  if (rows_per_split) *rows_per_split = rps;
  return (int)cdiv(cap, rps);
}

// candidate splits of the forward and dh launches: enough workgroups to fill the device several times over (the
// sweep is a chain of dependent tile loads: co-resident workgroups hide it), the dh slabs bounded
static int ksplits_of(int64_t cap, int64_t K, int64_t d) {
  const int64_t tiles = cdiv(cap, (int64_t)TS), nkt = cdiv(K, (int64_t)TS);
  int64_t ks = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, nkt), cdiv(1024, tiles)));
  while (ks > 1 && ks * cap * d * 4 > ((int64_t)64 << 20)) --ks;
  return (int)cdiv(nkt, cdiv(nkt, ks));               // no empty split
}

// the workspace, in floats: lse [cap] | z0 [cap] | pm [ks][cap] | ps [ks][cap] | part (double) [nb][2] | dEc slabs
struct WsLayout {
  int ks, sp;
  int64_t nb, pm, ps, part, slab, total;
};

static WsLayout ws_layout(int64_t cap, int64_t K, int64_t d) {
  WsLayout L;
  L.ks = ksplits_of(cap, K, d);
  L.sp = splits_of(cap, K, nullptr);
  L.nb = cdiv(cap, (int64_t)256);
  L.pm = 2 * cap;
  L.ps = L.pm + (int64_t)L.ks * cap;
  L.part = (L.ps + (int64_t)L.ks * cap + 1) / 2 * 2;
  L.slab = (L.part + 4 * L.nb + 3) / 4 * 4;
  L.total = L.slab + (L.sp > 1 ? (int64_t)L.sp * K * d : 0);
  return L;
}

static bool supported(int dtype, int64_t d, int64_t K) {
  if (dtype != RS_DTYPE_F32 && dtype != RS_DTYPE_BF16) return false;
  if (d < 1 || d > GEN_DMAX || (dtype == RS_DTYPE_BF16 && d % 8)) return false;
  return K >= 1 && K <= KMAX;
}

static bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// the rs_sce_head_* entries: bf16 rows up to WIDE_DMAX take the MFMA sweep (DP = 256)
constexpr int64_t WIDE_DMAX = 256;

static bool on_sweep(int dtype, int64_t d, bool wide) {
  return d <= 128 || (wide && dtype == RS_DTYPE_BF16 && d <= WIDE_DMAX);
}

// items: the stationary items (rows or candidates); ysplits: the splits of the swept side
template <int MODE>
static void launch(int dtype, int64_t d, int64_t items, int ysplits, hipStream_t s, const Args& a, bool wide) {
  const bool bf = dtype == RS_DTYPE_BF16;
  if (!on_sweep(dtype, d, wide)) {                   // one workgroup per item
    const dim3 grid((unsigned)items, (unsigned)ysplits);
    if (bf) hipLaunchKernelGGL((generic_kernel<__bf16, MODE>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((generic_kernel<float, MODE>), grid, dim3(256), 0, s, a);
    return;
  }
  const dim3 grid((unsigned)cdiv(items, (int64_t)TS), (unsigned)ysplits);
  if (bf) {
    if (d <= 64) hipLaunchKernelGGL((sweep_kernel<__bf16, 64, MODE>), grid, dim3(256), 0, s, a);
    else if (d <= 128) hipLaunchKernelGGL((sweep_kernel<__bf16, 128, MODE>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((sweep_kernel<__bf16, 256, MODE>), grid, dim3(256), 0, s, a);
  } else {
    if (d <= 64) hipLaunchKernelGGL((sweep_kernel<float, 64, MODE>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((sweep_kernel<float, 128, MODE>), grid, dim3(256), 0, s, a);
  }
}

static int fwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab, const int32_t* count,
               const void* E, const float* bias, const float* logq, int64_t V1, const int64_t* cand, int64_t K,
               const float* divisor, void* ws, float* out, void* stream, bool wide) {
  if (!supported(dtype, d, K)) return RS_ERR_UNSUPPORTED;
  if (cap <= 0 || cap >= ((int64_t)1 << 31) || V1 < 1 || V1 >= ((int64_t)1 << 31) || !hl || !lab || !E || !cand ||
      !divisor || !ws || !out || ldh < d || !al16(ws))
    return RS_ERR_ARG;
  const int64_t sz = dtype == RS_DTYPE_BF16 ? 2 : 4;
  Args a = {};
  a.hl = hl; a.ldh = ldh; a.lab = lab; a.cnt = count; a.cap = cap; a.E = E; a.V1 = V1; a.cand = cand; a.K = K;
  a.d = (int)d;
  a.bias = bias;
  a.logq = logq;
  a.vec = al16(hl) && al16(E) && (ldh * sz) % 16 == 0 && (d * sz) % 16 == 0;
  const WsLayout L = ws_layout(cap, K, d);
  a.lse = (float*)ws;
  a.z0 = a.lse + cap;
  a.pm = a.lse + L.pm;
  a.ps = a.lse + L.ps;
  double* part = (double*)(a.lse + L.part);
  hipStream_t s = (hipStream_t)stream;
  launch<FWD>(dtype, d, cap, L.ks, s, a, wide);
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)L.nb), dim3(256), 0, s, a.pm, a.ps, L.ks, lab, count, cap, V1,
                     a.z0, a.lse, part);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, s, part, L.nb, divisor, out);
  return (int)hipGetLastError();
}

static int bwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab, const int32_t* count,
               const void* E, const float* bias, const float* logq, int64_t V1, const int64_t* cand, int64_t K,
               const float* divisor, const float* dloss, void* ws, float* dh, float* coef, float* pg, float* dEc,
               float* dbc, int64_t* keys, void* stream, bool wide) {
  if (!supported(dtype, d, K)) return RS_ERR_UNSUPPORTED;
  if (cap <= 0 || cap >= ((int64_t)1 << 31) || V1 < 1 || V1 >= ((int64_t)1 << 31) || !hl || !lab || !E || !cand ||
      !divisor || !ws || !dh || !coef || !pg || !dEc || ldh < d || !al16(ws))
    return RS_ERR_ARG;
  const int64_t sz = dtype == RS_DTYPE_BF16 ? 2 : 4;
  Args a = {};
  a.hl = hl; a.ldh = ldh; a.lab = lab; a.cnt = count; a.cap = cap; a.E = E; a.V1 = V1; a.cand = cand; a.K = K;
  a.d = (int)d;
  a.bias = bias;
  a.logq = logq;
  a.vec = al16(hl) && al16(E) && (ldh * sz) % 16 == 0 && (d * sz) % 16 == 0;
  a.lse = (float*)ws;
  a.z0 = a.lse + cap;
  a.div = divisor; a.dloss = dloss; a.dh = dh; a.coef = coef; a.pg = pg;
  const WsLayout L = ws_layout(cap, K, d);
  const int sp = splits_of(cap, K, &a.rows_per_split);
  a.slab = sp > 1 ? a.lse + L.slab : dEc;
  if (bias) a.dbslab = sp > 1 ? a.lse + (L.total + 3) / 4 * 4 : dbc;
  hipStream_t s = (hipStream_t)stream;
  launch<DH>(dtype, d, cap, L.ks, s, a, wide);
  launch<DEC>(dtype, d, K, sp, s, a, wide);
  if (sp > 1) {
    hipError_t e = launch_reduce_slabs(a.slab, sp, K * d, K * d, dEc, nullptr, 0, s);
    if (e != hipSuccess) return (int)e;
    if (bias && (e = launch_reduce_slabs(a.dbslab, sp, K, K, dbc, nullptr, 0, s)) != hipSuccess) return (int)e;
  }
  if (keys)
    hipLaunchKernelGGL(keys_kernel, dim3((unsigned)cdiv(cap + K, (int64_t)256)), dim3(256), 0, s, lab, count, cap,
                       cand, K, V1, keys);
  return (int)hipGetLastError();
}

// the rs_sce_head_* workspace, in floats: the layout above, then the dbc row-split slabs [sp][K] (with a bias)
static int64_t head_ws_total(int64_t cap, int64_t K, int64_t d, bool has_bias) {
  const WsLayout L = ws_layout(cap, K, d);
  return has_bias && L.sp > 1 ? (L.total + 3) / 4 * 4 + (int64_t)L.sp * K : L.total;
}

}  // namespace sce

extern "C" {

int64_t rs_sas_sce_max_k(void) { return sce::KMAX; }

int64_t rs_sas_sce_ws_bytes(int64_t cap, int64_t K, int64_t d) {
  if (cap <= 0 || K <= 0 || d <= 0) return -1;
  return 4 * sce::ws_layout(cap, K, d).total;
}

int64_t rs_sas_sce_dh_splits(int64_t cap, int64_t K, int64_t d) {
  if (cap <= 0 || K <= 0 || d <= 0) return -1;
  return sce::ksplits_of(cap, K, d);
}

int rs_sas_sce_fwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                   const int32_t* count, const void* E, int64_t V1, const int64_t* cand, int64_t K,
                   const float* divisor, void* ws, float* out, void* stream) {
  return sce::fwd(dtype, cap, d, hl, ldh, lab, count, E, nullptr, nullptr, V1, cand, K, divisor, ws, out, stream,
                  false);
}

int rs_sas_sce_bwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                   const int32_t* count, const void* E, int64_t V1, const int64_t* cand, int64_t K,
                   const float* divisor, const float* dloss, void* ws, float* dh, float* coef, float* pg, float* dEc,
                   int64_t* keys, void* stream) {
  return sce::bwd(dtype, cap, d, hl, ldh, lab, count, E, nullptr, nullptr, V1, cand, K, divisor, dloss, ws, dh, coef,
                  pg, dEc, nullptr, keys, stream, false);
}

int64_t rs_sce_head_ws_bytes(int dtype, int64_t cap, int64_t K, int64_t d, int has_bias) {
  if (cap <= 0 || K <= 0 || !sce::supported(dtype, d, K)) return -1;
  return 4 * sce::head_ws_total(cap, K, d, has_bias != 0);
}

int64_t rs_sce_head_dh_splits(int dtype, int64_t cap, int64_t K, int64_t d) {
  if (cap <= 0 || K <= 0 || !sce::supported(dtype, d, K)) return -1;
  return sce::ksplits_of(cap, K, d);
}

int rs_sce_head_path(int dtype, int64_t d) {
  if (!sce::supported(dtype, d, 1)) return -1;
  return sce::on_sweep(dtype, d, true) ? 1 : 0;
}

int rs_sce_head_fwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                    const int32_t* count, const void* E, const float* bias, int64_t V1, const int64_t* cand, int64_t K,
                    const float* divisor, void* ws, float* out, void* stream) {
  return sce::fwd(dtype, cap, d, hl, ldh, lab, count, E, bias, nullptr, V1, cand, K, divisor, ws, out, stream, true);
}

int rs_sce_head_bwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                    const int32_t* count, const void* E, const float* bias, int64_t V1, const int64_t* cand, int64_t K,
                    const float* divisor, const float* dloss, void* ws, float* dh, float* coef, float* pg, float* dEc,
                    float* dbc, int64_t* keys, void* stream) {
  if (!bias != !dbc) return sce::supported(dtype, d, K) ? RS_ERR_ARG : RS_ERR_UNSUPPORTED;
  return sce::bwd(dtype, cap, d, hl, ldh, lab, count, E, bias, nullptr, V1, cand, K, divisor, dloss, ws, dh, coef, pg,
                  dEc, dbc, keys, stream, true);
}

int rs_sce_head_logq_fwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                         const int32_t* count, const void* E, const float* bias, const float* logq, int64_t V1,
                         const int64_t* cand, int64_t K, const float* divisor, void* ws, float* out, void* stream) {
  return sce::fwd(dtype, cap, d, hl, ldh, lab, count, E, bias, logq, V1, cand, K, divisor, ws, out, stream, true);
}

int rs_sce_head_logq_bwd(int dtype, int64_t cap, int64_t d, const void* hl, int64_t ldh, const int64_t* lab,
                         const int32_t* count, const void* E, const float* bias, const float* logq, int64_t V1,
                         const int64_t* cand, int64_t K, const float* divisor, const float* dloss, void* ws, float* dh,
                         float* coef, float* pg, float* dEc, float* dbc, int64_t* keys, void* stream) {
  if (!bias != !dbc) return sce::supported(dtype, d, K) ? RS_ERR_ARG : RS_ERR_UNSUPPORTED;
  return sce::bwd(dtype, cap, d, hl, ldh, lab, count, E, bias, logq, V1, cand, K, divisor, dloss, ws, dh, coef, pg,
                  dEc, dbc, keys, stream, true);
}

int rs_alias_items(const uint64_t* seed_base, uint64_t salt, const uint64_t* table, int64_t item_num, int64_t K,
                   int64_t* out, void* stream) {
  if (item_num < 1 || item_num >= ((int64_t)1 << 32) || K < 1 || !table || !out) return RS_ERR_ARG;
  hipLaunchKernelGGL(sce::alias_items_kernel, dim3((unsigned)cdiv(K, (int64_t)256)), dim3(256), 0,
                     (hipStream_t)stream, seed_base, salt, table, item_num, K, out);
  return (int)hipGetLastError();
}

int rs_uniform_items(const uint64_t* seed_base, uint64_t salt, int64_t item_num, int64_t K, int64_t* out, void* stream) {
  if (item_num <= 0 || K <= 0 || !out) return RS_ERR_ARG;
  hipLaunchKernelGGL(sce::uniform_items_kernel, dim3((unsigned)cdiv(K, (int64_t)256)), dim3(256), 0,
                     (hipStream_t)stream, seed_base, salt, item_num, K, out);
  return (int)hipGetLastError();
}

}  // extern "C"
