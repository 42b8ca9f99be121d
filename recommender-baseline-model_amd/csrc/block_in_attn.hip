// The first SAS block's input chain and its attention forward in one launch (bf16, d in {64, 128}, one head):
// the kernel behind rs_sas_block_in_attn.
//
// rs_sas_block_in (embed form) followed by rs_attn_fwd is a launch boundary across which every attention workgroup
// reloads the K/V image the previous launch just stored.  Block 0's K and V rows are a row-local function of the
// batch (embedding -> scale + position -> dropout -> timeline mask -> x Wkv^T + bkv), so each of the nsplit attention
// workgroups of a sequence forms the image in its own LDS, with the row chain's own stages (rowchain.hip embed_tile,
// fwd_in_kv_half(2), fwd_in_q_x) and then runs the forward's tile body (attention_lds.hip attn_fwd_tile) on it: the same
// operations on the same rounded values, so every output is bit for bit the two launches'.
//
//  * grid, coordinates, XCD placement: the attention forward's (block_coords; nsplit workgroups per sequence);
//  * K/V phase: the workgroup needs tiles 0 .. its last query tile.  Wave w takes its own query tile
//    (split + w nsplit) and at most one more (two for a wave without a query tile): <= 2 x tiles, kept in registers
//    across the phases; a wave with two runs both through one pass over the weight fragments (rowchain.hip mm2: the
//    projections are bound by LDS fragment reads).  Rounded k / v rows go into the LDS images in attn_fwd_lds_kernel's
//    layout (Img<D>, rows past T zero, as stage2 leaves them);
//  * Q phase (after the K phase, before the V phase): fwd_in_q_x on the wave's own query tile; the rounded q IS the attention's B fragment (lane (g, cl) holds
//    columns 32s + 8g .. + 7 of row cl in both layouts), so it reaches attn_fwd_tile in registers;
//  * who stores what: tile t belongs to the workgroup of split t % nsplit, which stores x0, kv, Q, mean, rstd, q, o,
//    lse and counts the tile's positions; the copies of a tile the other workgroups form stay in their LDS;
//  * LDS: the V image's place is free until the V phase, so Wk and Wq are staged THERE at the start (the region is
//    sized for whichever is larger) and Wv in a slot of its own: all three weight images are requested once, with the
//    embedding gathers, and nothing is re-staged.  K phase and Q phase (weights in the V region) -> barrier -> V phase
//    (writes the V image over them) -> barrier -> attention.  At d = 128, T = 200: 58.5 KB K image + 64 KB shared
//    region + 32 KB Wv + vectors = 157 KB;
//  * no workgroup waits on another: barriers within the workgroup only.
#define RC_DEVICE_ONLY
#include "rowchain.hip"
#define ATTN_LDS_DEVICE_ONLY
#include "attention_lds.hip"

// attention_lds.hip's host side (that translation unit)
int attn_lds_fwd_nsplit(int64_t BH, int64_t T);
bool attn_lds_supported(int64_t T, int64_t Dh);

namespace ia {

using rc::Lay;
using rc::Raw;
using rc::Tile;

constexpr int WAVES = 8;   // both kernels' workgroup: 8 waves

template <int D> struct Slots {
  static constexpr int WB = Lay<D>::WBYTES;
  static constexpr size_t STATIC = (size_t)WB + 5 * D * 4 + WAVES * 4;   // Wv, the vectors, the waves' counts
};
// image rows: keys 0 .. 16 nq - 1; the V image up to the next multiple of 32 (tr_frag reads 32-row steps)
static __host__ __device__ inline int k_rows(int nq) { return 16 * nq; }
static __host__ __device__ inline int v_rows(int nq) { return 32 * ((nq + 1) / 2); }
// dynamic LDS: the K image, then the region that holds Wk, Wq first and the V image + key flags afterwards
template <int D> static size_t dyn_lds_bytes(int T) {
  const int nq = (T + 15) / 16;
  const size_t v = (size_t)v_rows(nq) * Img<D>::LD * 2 + (size_t)v_rows(nq) * 4, w = 2 * (size_t)Slots<D>::WB;
  return (size_t)k_rows(nq) * Img<D>::LD * 2 + (v > w ? v : w);
}

// tile t of sequence b: rows b T + 16 t + cl (rows past the sequence's end are not ok and read its last row)
__device__ __forceinline__ Tile seq_tile(int64_t b, int T, int t, int cl) {
  Tile x;
  const int row = 16 * t + cl;
  x.ok = row < T;
  x.m = b * T + row;
  x.mc = x.ok ? x.m : b * T + T - 1;
  return x;
}
// the i-th tile (ascending) of 0 .. ntile - 1 that is not a query tile of this split, or -1
__device__ __forceinline__ int other_tile(int i, int split, int ns, int ntile) {
  if (ns == 1) return -1;
  const int j = i % (ns - 1), t = (i / (ns - 1)) * ns + (j < split ? j : j + 1);
  return t < ntile ? t : -1;
}
// a tile's rounded rows into an image (zero where the row is past T)
template <int D>
__device__ __forceinline__ void put_rows(bf16* img, int t, const Raw<D>& r, bool ok, int g, int cl) {
  bf16* p = img + (16 * t + cl) * Img<D>::LD + 8 * g;
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
#pragma unroll
  for (int s = 0; s < Lay<D>::S; ++s) *reinterpret_cast<bf16x8*>(p + 32 * s) = ok ? r.v[s] : z;
}


// The two argument sets hold more pointers than the scalar registers keep at once (rowchain.hip, TurnArgs): they are
// ONE struct, and the attention's late ones (lse, out, the dropout seed) are read from the kernel-argument segment
// where the attention phase starts, through a pointer the optimizer cannot see through.
struct Args {
  rs_sas_in_args in;
  AttnLdsArgs a;
  int ncount;
};
typedef const __attribute__((address_space(4))) Args* ArgsPtr;
__device__ __forceinline__ ArgsPtr args_late() {
  ArgsPtr kp = (ArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();   // explicit arguments start at offset 0
  asm volatile("" : "+s"(kp));
  return kp;
}

template <int D>
__global__ __launch_bounds__(64 * WAVES) void block_in_attn_kernel(Args k) {
  const rs_sas_in_args& in = k.in;
  const int ncount = k.ncount;
  AttnLdsArgs a = {};   // the early fields; the rest follow late
  a.B = k.a.B, a.T = k.a.T, a.H = 1, a.nsplit = k.a.nsplit;
  typedef Slots<D> SL;
  constexpr int LD = Img<D>::LD, KC = D / 32;
  __shared__ __attribute__((aligned(16))) char wv[SL::WB];
  __shared__ __attribute__((aligned(16))) float lv[5 * D];   // ln1_w, ln1_b, bq, bk, bv
  __shared__ int wcnt[WAVES];
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4,
            cl = lane & 15;
  int64_t b;   // one head: the sequence-head index is the sequence
  int split;
  block_coords(a, b, split);
  const int T = (int)a.T, nq = (T + 15) / 16, ns = a.nsplit;
  const int ntile = last_tile_of_split(nq, split, ns) + 1;   // K/V tiles 0 .. the split's last query tile
  bf16* Ks = reinterpret_cast<bf16*>(smem);
  bf16* Vs = Ks + k_rows(nq) * LD;
  float* km = reinterpret_cast<float*>(Vs + v_rows(nq) * LD);
  char* wk = reinterpret_cast<char*>(Vs);   // until the V phase: Wk, Wq where the V image and the key flags will be
  char* wq = wk + SL::WB;
  // this wave's tiles: A = its query tile where it has one (the only tile it stores), else another; B = one more.
  // The tiles that are no query tile of this split go, ascending, to waves 7, 6, ..., 0, 7, ...: with at most 16
  // tiles a wave gets at most two (a wave with a query tile at most one more)
  const int qt = split + wave * ns;
  const bool hasq = qt < nq;
  const int oA = other_tile(WAVES - 1 - wave, split, ns, ntile);
  const int tA = hasq ? qt : oA, tB = hasq ? oA : other_tile(2 * WAVES - 1 - wave, split, ns, ntile);
  const bool hasA = tA >= 0, hasB = tB >= 0;
  const Tile TA = seq_tile(b, T, hasA ? tA : 0, cl), TB = seq_tile(b, T, hasB ? tB : 0, cl);
  const rs_sas_embed_args& e = in.e;
  const uint32_t es32 = e.drop_p > 0.f ? seed32(eff_seed(e.salt, e.seed_base)) : 0u;
  // the x tiles (as block_in_kernel's load_x: the count's id goes out with the gathers)
  Raw<D> xa, xb;
  int cnt = 0;
  {
    const int64_t cid = e.count_ids && hasq && TA.ok && g == 0 ? e.count_ids[TA.mc] : 0;
    if (hasA) rc::embed_tile<D>(xa, e, TA, es32, g);
    if (hasB) rc::embed_tile<D>(xb, e, TB, es32, g);
    if (e.count_ids) cnt = __popcll(__ballot(cid != 0));
    if (hasq) rc::store_raw<D>(e.x0, D, TA.m, TA.ok, xa, g);
  }
  rc::stage_slot<D>(wk, in.Wkv, D, wave, lane);
  rc::stage_slot<D>(wq, in.Wq, D, wave, lane);
  rc::stage_slot<D>(wv, in.Wkv + (int64_t)D * D, D, wave, lane);
  {
    const float* const V[5] = {in.ln_w, in.ln_b, in.bq, in.bkv, in.bkv + D};
    rc::stage_v<D, 5>(lv, V, tid);
  }
  if (lane == 0) wcnt[wave] = cnt;
  __syncthreads();
  if (e.count_parts && tid == 0) {   // integer counts: exact in any order; every slot of count_parts is written once
    int c = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) c += wcnt[w];
    const int64_t nwg = (int64_t)ns * a.B, lin = blockIdx.x + (int64_t)ns * blockIdx.y;
    e.count_parts[lin] = c;
    for (int64_t i = lin + nwg; i < ncount; i += nwg) e.count_parts[i] = 0;
  }
  // K phase (kv rows are stored through a tile that is ok only where this workgroup owns the row)
  Tile SA = TA, SB = TB;
  SA.ok = TA.ok && hasq;
  SB.ok = false;
  Raw<D> r;
  if (hasB) {   // two tiles: each weight fragment is read once for both
    Raw<D> r2;
    rc::fwd_in_kv_half2<D>(xa, xb, SA, SB, rc::wimg(wk), lv, in.kv, 0, lane, r, r2);
    put_rows<D>(Ks, tA, r, TA.ok, g, cl);
    put_rows<D>(Ks, tB, r2, TB.ok, g, cl);
  } else if (hasA) {
    rc::fwd_in_kv_half<D>(xa, SA, rc::wimg(wk), lv, in.kv, 0, lane, r);
    put_rows<D>(Ks, tA, r, TA.ok, g, cl);
  }
  // Q phase: the rounded q is the attention's B fragment (rows past T zero, as gload8 hands them to the forward)
  bf16x8 qf[KC];
  if (hasq) {
    rc::fwd_in_q_x<D>(xa, TA, rc::wimg(wq), lv, in.eps, in.Q, in.mean, in.rstd, in.q, lane, r);
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      typedef __attribute__((ext_vector_type(4))) unsigned u4;
      u4 v = __builtin_bit_cast(u4, r.v[kc]);
      v &= TA.ok ? 0xffffffffu : 0u;
      qf[kc] = __builtin_bit_cast(bf16x8, v);
    }
  }
  __syncthreads();   // every wave is past Wk and Wq: their place becomes the V image
  asm volatile("" ::: "memory");   // no hoisting across the phases (registers)
  // causal: no key-padding flags; the V rows past the last tile that the last 32-row step reads are zero
  for (int i = tid; i < v_rows(nq); i += 64 * WAVES) km[i] = 0.f;
  if (ntile & 1) {
    bf16x8 z;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) z[kk] = (bf16)0.f;
    for (int i = tid; i < 16 * LD / 8; i += 64 * WAVES) reinterpret_cast<bf16x8*>(Vs + 16 * ntile * LD)[i] = z;
  }
  // V phase
  if (hasB) {   // two tiles: each weight fragment is read once for both
    Raw<D> r2;
    rc::fwd_in_kv_half2<D>(xa, xb, SA, SB, rc::wimg(wv), lv, in.kv, 1, lane, r, r2);
    put_rows<D>(Vs, tA, r, TA.ok, g, cl);
    put_rows<D>(Vs, tB, r2, TB.ok, g, cl);
  } else if (hasA) {
    rc::fwd_in_kv_half<D>(xa, SA, rc::wimg(wv), lv, in.kv, 1, lane, r);
    put_rows<D>(Vs, tA, r, TA.ok, g, cl);
  }
  __syncthreads();   // the images are complete
  asm volatile("" ::: "memory");
  if (!hasq) return;   // no barrier follows
  // the attention forward's tile body
  {
    const ArgsPtr kp = args_late();
    a.out = kp->a.out, a.ldout = kp->a.ldout, a.lse = kp->a.lse, a.scale = kp->a.scale, a.mask_kind = 0;
    a.drop_p = kp->a.drop_p, a.seed = kp->a.seed, a.seed_base = kp->a.seed_base;
  }
  const uint64_t seed = eff_seed(a.seed, a.seed_base);
  if (wave >= WAVES / 2) __builtin_amdgcn_s_setprio(1);   // as attn_fwd_lds_kernel
  attn_fwd_tile<D>(a, Ks, Vs, km, qf, qt, b, b, 0, T, nq, seed, lane);
}

// ------------------------------------------------------------------ host side
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// 0: the fused launch covers (d, B, T) -- *nsplit = its workgroups per sequence, *lds = its dynamic LDS bytes
static int plan(int64_t d, int64_t B, int64_t T, int* nsplit, size_t* lds) {
  if (d != 64 && d != 128) return RS_ERR_UNSUPPORTED;
  if (B <= 0 || T <= 0) return RS_ERR_ARG;
  // what sends rs_attn_fwd to the LDS kernel (attention.hip use_lds_path)
  if (!attn_lds_supported(T, d) || B * T * (T + (T & 1)) >= ((int64_t)1 << 32)) return RS_ERR_UNSUPPORTED;
  const int ns = attn_lds_fwd_nsplit(B, T), nq = (int)((T + 15) / 16);
  if (ns > nq || (nq + ns - 1) / ns > WAVES) return RS_ERR_UNSUPPORTED;   // one query tile per wave
  const size_t dyn = d == 64 ? dyn_lds_bytes<64>((int)T) : dyn_lds_bytes<128>((int)T);
  const size_t stat = d == 64 ? Slots<64>::STATIC : Slots<128>::STATIC;
  if (dyn + stat > 160 * 1024) return RS_ERR_UNSUPPORTED;
  *nsplit = ns;
  *lds = dyn;
  return 0;
}

template <int D>
static int launch(const rs_sas_in_args& in, const AttnLdsArgs& a, int ncount, size_t lds, hipStream_t s) {
  const void* fn = reinterpret_cast<const void*>(block_in_attn_kernel<D>);
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const Args k = {in, a, ncount};
  hipLaunchKernelGGL((block_in_attn_kernel<D>), dim3((unsigned)a.nsplit, (unsigned)a.B), dim3(64 * WAVES), lds, s, k);
  return (int)hipGetLastError();
}

}  // namespace ia

extern "C" {

int rs_sas_block_in_attn_nsplit(int64_t d, int64_t B, int64_t T) {
  int ns = 0;
  size_t lds = 0;
  return ia::plan(d, B, T, &ns, &lds) == 0 ? ns : 0;
}

int rs_sas_block_in_attn(int64_t d, const rs_sas_in_attn_args* k, void* stream) {
  if (!k || k->in.M <= 0 || k->B <= 0) return RS_ERR_ARG;
  const rs_sas_in_args& in = k->in;
  const rs_sas_embed_args& e = in.e;
  if (e.T <= 0 || k->B * e.T != in.M) return RS_ERR_ARG;
  if (!e.ids || !e.item_emb || !e.pos_emb || !e.x0 || !e.count_ids != !e.count_parts) return RS_ERR_ARG;
  if (!in.ln_w || !in.ln_b || !in.Q || !in.mean || !in.rstd || !in.Wq || !in.bq || !in.q || !in.Wkv || !in.bkv ||
      !in.kv || !k->o || !k->lse)
    return RS_ERR_ARG;
  if (!ia::aligned16(e.item_emb) || !ia::aligned16(e.pos_emb) || !ia::aligned16(e.x0) || !ia::aligned16(in.Q) ||
      !ia::aligned16(in.q) || !ia::aligned16(in.kv) || !ia::aligned16(in.Wq) || !ia::aligned16(in.Wkv) ||
      !ia::aligned16(k->o))
    return RS_ERR_ARG;
  int ns = 0;
  size_t lds = 0;
  const int pc = ia::plan(d, k->B, e.T, &ns, &lds);
  if (pc) return pc;
  if (e.count_parts && k->ncount < (int64_t)ns * k->B) return RS_ERR_ARG;
  rs_sas_in_args a = in;
  a.x = e.x0;
  a.ldx = d;
  AttnLdsArgs t = {};
  t.B = k->B; t.T = e.T; t.H = 1;
  t.out = (bf16*)k->o; t.ldout = d; t.lse = k->lse; t.scale = k->scale; t.mask_kind = 0; t.ids = e.ids;
  t.drop_p = k->drop_p; t.seed = k->salt; t.seed_base = e.seed_base; t.nsplit = ns;
  const int nc = (int)(k->ncount < 0x7fffffff ? k->ncount : 0x7fffffff);
  return d == 64 ? ia::launch<64>(a, t, nc, lds, (hipStream_t)stream)
                 : ia::launch<128>(a, t, nc, lds, (hipStream_t)stream);
}

}  // extern "C"
