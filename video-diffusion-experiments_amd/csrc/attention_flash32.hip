// Small-head flash attention on v_mfma_f32_32x32x16_bf16 (d = 40: SD-1.5's
// level-1 spatial self-attention, the hottest attention of the step).
//
//   S^T = K'.Q'^T   A = K rows (32 keys x 16 d, ds_read_b128), B = Q'^T from
//                   registers; contraction over d padded to DK = 48 (3 MFMAs
//                   per 32x32 tile instead of 4 with 16x16x32 at 64).  Column D
//                   of K' holds 1.0 and column D of Q' holds -mu (mu = this
//                   query's running max, bf16-representable), so the MFMA emits
//                   x = s - mu directly.  When the caller folded the softmax
//                   scale and log2(e) into its Q projection (c == 1, the model
//                   path: vdiff Attention.prepare) p = exp2(x) needs no per-score
//                   FMA; otherwise p = exp2(c*x) (one multiply).
//   O^T += V^T.P^T  the S^T accumulator, packed to bf16, IS the P^T B operand
//                   (cdna_hip_programming.md §3 "accumulator tile as the next
//                   MFMA's operand"; permuted key order within each 16-key
//                   step), V^T comes from ds_read_b64_tr_b16 in that order; V's
//                   column D holds 1.0 so the same MFMA yields the row sum.
// Deferred max (T13): while every u of the tile is <= THR, p = exp2(u) (one
// v_exp + 1/2 v_max3 + 1/2 v_cvt_pk per score); otherwise (first tile, or a
// row max that grew by > THR) mu is raised for those rows, the tile's u and
// the O rows are rescaled and Q''s -mu entry is rewritten — the decision covers
// the whole tile before any of its P is formed, so nothing is half-scaled.
// P <= 2^THR stays exact in the fp32 O/l accumulators; P's bf16 rounding is
// relative, so the normalised result does not depend on THR.
// Layout: 4 waves x 64 queries (2 query blocks of 32); K/V tiles of 64 keys
// double-buffered in ONE LDS array (K rows padded to 56 elements, V as
// [2][64 keys][32 d] images): both the K b128 reads and the V transposed reads
// are bank-conflict free (tools/lds_banks.py).  Register staging (T14): the
// next tile's global loads issue before this tile's MFMAs, their LDS writes
// after the PV, one barrier per tile.  Epilogue: permlane32_swap pairs give
// 16-byte stores of 8 consecutive output channels.
#include "attention_common.h"

namespace {

// One pass of flash32's key loop (prologue tile load included).  EXACT tracks the
// running max of every tile (deferred, THR); the fast pass computes it for the
// first tile only and afterwards lets P grow up to 2^32 before raising mu by
// log2(row sum) — the row sum comes free from the PV MFMA's ones column, so the
// common tile has no max reduction at all (-40 VALU ops per 64 keys).  mu stays
// >= the running max (l >= 2^(max - mu)), so nothing underflows that matters;
// a row sum >= 2^100 (or non-finite) means a score jumped past the fp32/bf16
// range and the pass reports `bad` so the block reruns EXACT.
template <int D, bool UNITC, bool EXACT, int QB = 2>
__device__ __forceinline__ bool f32_loop(bf16_t* lds, const bf16_t* kb_ptr, const bf16_t* vb_ptr, int ldk32,
                                         int ldv32, int64_t skv, const int (&krow)[F32Cfg<D>::LREG],
                                         const uint32_t (&kcol)[F32Cfg<D>::LREG],
                                         const uint32_t (&ldsk)[F32Cfg<D>::LREG],
                                         const uint32_t (&ldsv)[F32Cfg<D>::LREG],
                                         bf16x8 (&qf)[QB][F32Cfg<D>::KSTEPS], f32x16 (&oacc)[F32Cfg<D>::NDB][QB],
                                         int r32, int hh, int vtr, float c) {
  using C = F32Cfg<D>;
  constexpr float RESCALE = 4294967296.0f;        // 2^32
  constexpr float BAD = 1.2676506002282294e30f;   // 2^100
#pragma unroll
  for (int db = 0; db < C::NDB; ++db)
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[db][qb][i] = 0.f;
  float mu[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) mu[qb] = 0.f;
  bool bad = false;

  const int ntiles = (int)((skv + KT - 1) / KT);
  const bool ragged = (skv % KT) != 0;
  stage_t<C::LREG> kvst = kv_load<C::LREG>(kb_ptr, vb_ptr, ldk32, ldv32, 0, skv, krow, kcol);
#pragma unroll
  for (int i = 0; i < C::LREG; ++i) {
    *(uint4*)(lds + ldsk[i]) = make_uint4(kvst[4 * i], kvst[4 * i + 1], kvst[4 * i + 2], kvst[4 * i + 3]);
    *(uint4*)(lds + ldsv[i]) = make_uint4(kvst[4 * C::LREG + 4 * i], kvst[4 * C::LREG + 4 * i + 1],
                                          kvst[4 * C::LREG + 4 * i + 2], kvst[4 * C::LREG + 4 * i + 3]);
  }
  __syncthreads();

  // one K/V tile: the general form (tile max on tile 0 / every tile of the exact pass,
  // ragged-key masking, rescale one tile late)
  auto tile_generic = [&](int t) {
    const int buf = t & 1;
    if (t + 1 < ntiles) kvst = kv_load<C::LREG>(kb_ptr, vb_ptr, ldk32, ldv32, t + 1, skv, krow, kcol);
    const bf16_t* kl = lds + buf * C::STAGE;
    const bf16_t* vl = kl + C::K_ELEMS;
    // ---- x^T = K'.Q'^T  (= s - mu)
    f32x16 s[2][QB];
    bf16x8 kfr[2][C::KSTEPS];  // all K fragments of the tile first: one LDS latency, not six
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ks = 0; ks < C::KSTEPS; ++ks)
        kfr[kb][ks] = *(const bf16x8*)(kl + (kb * 32 + r32) * C::KS + ks * 16 + 8 * hh);
    __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead (the scheduler sinks them to their MFMAs)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int ks = 0; ks < C::KSTEPS; ++ks) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
          if (ks == 0) {
            f32x16 z;
#pragma unroll
            for (int i = 0; i < 16; ++i) z[i] = 0.f;
            s[kb][qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[kb][ks], qf[qb][ks], z, 0, 0, 0);
          } else {
            s[kb][qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[kb][ks], qf[qb][ks], s[kb][qb], 0, 0, 0);
          }
        }
      }
    }
    if (ragged && t == ntiles - 1) {  // keys past skv: x = -inf (rows are clamped duplicates)
      const int kvalid = (int)(skv - (int64_t)t * KT);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
          if (key >= kvalid) {
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) s[kb][qb][i] = -INFINITY;
          }
        }
    }
    // V^T fragments for this tile's PV, issued now so their LDS latency hides
    // under the softmax VALU work (key order of each step: 16*s2 + 8*(j>>2) + 4*hh + (j&3))
    bf16x8 vfr[C::NDB][2][2];
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bf16_t* p0 = vl + (db * KT + kb * 32 + 16 * s2) * 32 + vtr;
          const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (bf16x4 __attribute__((address_space(3)))*)(p0));
          const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (bf16x4 __attribute__((address_space(3)))*)(p0 + 8 * 32));
          vfr[db][kb][s2] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
    __builtin_amdgcn_sched_barrier(0);
    if (EXACT || t == 0) {  // ---- tile max (deferred, THR): every tile on the exact pass, tile 0 on the fast one
      float tm[QB];
      bool need = t == 0;
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const float m = tile_max(s[0][qb], s[1][qb]);
        tm[qb] = vmax2(m, partner32(m));
        need |= (UNITC ? tm[qb] : tm[qb] * c) > F32_THR;
      }
      if (__any(need)) {  // wave-uniform: first tile or a row max moved by > THR
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
          const bool up = t == 0 || (UNITC ? tm[qb] : tm[qb] * c) > F32_THR;
          const float nmu = up ? (float)(__bf16)(mu[qb] + tm[qb]) : mu[qb];
          const float delta = nmu - mu[qb];  // exact: both bf16 values
          const float alpha = __builtin_amdgcn_exp2f(UNITC ? -delta : -delta * c);
          mu[qb] = nmu;
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) s[kb][qb][i] -= delta;
#pragma unroll
          for (int db = 0; db < C::NDB; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[db][qb][i] *= alpha;
          if (hh == C::MU_H) qf[qb][C::MU_KS][C::MU_J] = (__bf16)(-nmu);
        }
      }
    }
    if (!EXACT && t > 1) {
      // ---- fast pass: rescale from the row sum of tiles 0..t-1 when it outgrows 2^32.
      // Checked one tile late, after this tile's QK^T MFMAs are issued, so reading the PV
      // accumulator does not drain the MFMA pipe right behind the PV chain; this tile's
      // scores (formed with the old mu) take the same shift as the exact path's.
      float lq[QB];
      bool resc = false, over = false;
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const float lown = oacc[C::L_DB][qb][C::L_I];
        const float lp = partner32(lown);
        lq[qb] = hh == C::L_H ? lown : lp;
        resc |= lq[qb] > RESCALE;
        over |= !(lq[qb] < BAD);
      }
      if (__any(over)) {
        bad = true;
      } else if (__any(resc)) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
          const float step = lq[qb] > RESCALE ? __builtin_amdgcn_logf(lq[qb]) : 0.f;  // log2(l)
          const float nmu = (float)(__bf16)(mu[qb] + (UNITC ? step : step / c));
          const float delta = nmu - mu[qb];
          const float alpha = __builtin_amdgcn_exp2f(UNITC ? -delta : -delta * c);
          mu[qb] = nmu;
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) s[kb][qb][i] -= delta;
#pragma unroll
          for (int db = 0; db < C::NDB; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[db][qb][i] *= alpha;
          if (hh == C::MU_H) qf[qb][C::MU_KS][C::MU_J] = (__bf16)(-nmu);
        }
      }
    }
    // ---- P = exp2(x), packed: registers 8*s2 .. 8*s2+7 of tile kb = k-step (kb, s2)
    bf16x8 pf[2][2][QB];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          bf16x8 f;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            f[j] = (__bf16)__builtin_amdgcn_exp2f(UNITC ? s[kb][qb][8 * s2 + j] : s[kb][qb][8 * s2 + j] * c);
          pf[kb][s2][qb] = f;
        }
    // ---- O^T += V^T.P^T
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int qb = 0; qb < QB; ++qb)
            oacc[db][qb] =
                __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[db][kb][s2], pf[kb][s2][qb], oacc[db][qb], 0, 0, 0);
    if (t + 1 < ntiles) {
      bf16_t* nb = lds + (buf ^ 1) * C::STAGE;
#pragma unroll
      for (int i = 0; i < C::LREG; ++i) {
        *(uint4*)(nb + ldsk[i]) = make_uint4(kvst[4 * i], kvst[4 * i + 1], kvst[4 * i + 2], kvst[4 * i + 3]);
        *(uint4*)(nb + ldsv[i]) = make_uint4(kvst[4 * C::LREG + 4 * i], kvst[4 * C::LREG + 4 * i + 1],
                                             kvst[4 * C::LREG + 4 * i + 2], kvst[4 * C::LREG + 4 * i + 3]);
      }
    }
    __syncthreads();
  };
  for (int t = 0; t < ntiles; ++t) tile_generic(t);
  if (!EXACT) {  // the last tiles' row sums were not checked in the loop
    bool over = false;
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      const float lown = oacc[C::L_DB][qb][C::L_I];
      const float lp = partner32(lown);  // every lane takes part in the swap
      over |= !((hh == C::L_H ? lown : lp) < BAD);
    }
    bad |= __any(over);
  }
  return bad;
}

// QB = 32-query blocks per wave: 2 (256 VGPRs, two waves per SIMD; one block per wave with three
// waves per SIMD measured slower, 1010 vs 878 us: profiles/r02_attn_occupancy_ab.txt).
// FIX: flash40's exact fix-up pass — a 128-query block whose first output element is a NaN flag
// (flash40 found a score jump past its fast pass's range in the 512-query block around it)
// recomputes its queries with the exact pass.  Round 6: one workgroup per F32_FIXW blocks
// (fix_blocks in all), whose first F32_FIXW lanes read those blocks' flags at once (one load
// latency) and which then recomputes the flagged ones in turn — the launch that follows every
// flash40 call was one workgroup per block, 4096 at the level-1 self-attention, ~8 us with
// nothing flagged.  The fix-up runs QB = 1 (128-query blocks; a query's exact-pass arithmetic
// does not depend on QB): the block loop at QB = 2's 256 VGPRs spilled.  Every block has a flag
// of its own (flash40 writes one per 128 queries) and stores only its own rows, so the only
// block that overwrites a flag is the one that read it: which blocks share a workgroup, and the
// order the workgroups run in, do not matter (block ids start at an odd offset for every other
// head when ceil(sq / 128) is odd).
template <int D, bool UNITC, bool FIX = false, int QB = 2>
__global__ __launch_bounds__(NT, 2) void flash32_kernel(
    const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
    const bf16_t* __restrict__ v, int64_t ldv, bf16_t* __restrict__ o, int64_t ldo, int heads,
    int64_t sq, int64_t skv, int64_t kv_div, float c, int out_f32 = 0, int64_t fix_blocks = 0) {
  using C = F32Cfg<D>;
  __shared__ __attribute__((aligned(16))) bf16_t lds[2 * C::STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, hh = lane >> 5;
  // 1-D grid, XCD-aware (T1): the query blocks of one (image, head) get
  // consecutive logical ids and xcd_remap keeps consecutive ids on one XCD, so
  // that head's K/V is fetched into one L2 instead of eight.
  const int nqb = (int)((sq + 4 * 32 * QB - 1) / (4 * 32 * QB));
  auto flag_of = [&](int64_t lid) {  // the block's own flag: a NaN in its first output element
    const int qblk = (int)(lid % nqb);  // (first query of the block < sq, d 0 of its head)
    const int h = (int)((lid / nqb) % heads);
    const int64_t b = (lid / nqb) / heads;
    const int64_t f = (b * sq + (int64_t)qblk * (4 * 32 * QB)) * ldo + (int64_t)h * D;
    return out_f32 ? __builtin_isnan(((const float*)o)[f]) : ((o[f] & 0x7FFF) > 0x7F80);
  };
  auto block = [&](int lid) {
  const int qblk = lid % nqb;
  const int h = (lid / nqb) % heads;
  const int64_t b = (lid / nqb) / heads;
  const int64_t q0 = (int64_t)qblk * (4 * 32 * QB) + wave * (32 * QB);
  const int64_t bkv = b / kv_div;
  const bf16_t* qb_ptr = q + b * sq * ldq + (int64_t)h * D;
  const bf16_t* kb_ptr = k + bkv * skv * ldk + (int64_t)h * D;
  const bf16_t* vb_ptr = v + bkv * skv * ldv + (int64_t)h * D;

  // Q'^T fragments: lane holds Q'[q0 + qb*32 + r32][16*ks + 8*hh .. +7].  Q is
  // used as given (no bf16 prescale: that second rounding costs ~0.4% in P); with
  // UNITC the caller folded c into its Q projection (c == 1 exactly) and mu lives
  // in log2 units, otherwise mu is in raw score units and p = exp2(c * x).
  bf16x8 qf[QB][C::KSTEPS];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int64_t qi = q0 + qb * 32 + r32;
#pragma unroll
    for (int ks = 0; ks < C::KSTEPS; ++ks) {
      const int dd = ks * 16 + 8 * hh;
      uint4 u = make_uint4(0, 0, 0, 0);
      if (qi < sq && dd < D) u = *(const uint4*)(qb_ptr + qi * ldq + dd);
      qf[qb][ks] = __builtin_bit_cast(bf16x8, u);  // d = D entry starts at 0 (mu = 0)
    }
  }

  // LDS padding, written once: K' column D = 1.0 (the -mu column), V column D =
  // 1.0 (the row-sum column), every other padding element 0.
  for (int idx = tid; idx < 2 * KT; idx += NT) {
    const int buf = idx / KT, r = idx % KT;
    bf16_t* kl = lds + buf * C::STAGE;
    bf16_t* vl = kl + C::K_ELEMS;
    for (int cc = C::DCH; cc < C::DK / 8; ++cc)
      *(uint4*)(kl + r * C::KS + cc * 8) = make_uint4(cc == C::DCH ? 0x3F80u : 0u, 0, 0, 0);
    for (int cc = C::DCH; cc < C::DVP / 8; ++cc)
      *(uint4*)(vl + ((cc >> 2) * KT + r) * 32 + (cc & 3) * 8) = make_uint4(cc == C::DCH ? 0x3F80u : 0u, 0, 0, 0);
  }
  // staging slots (row, chunk) per thread, fixed for the kernel
  int krow[C::LREG];
  uint32_t kcol[C::LREG], ldsk[C::LREG], ldsv[C::LREG];
#pragma unroll
  for (int i = 0; i < C::LREG; ++i) {
    const int idx = (tid + i * NT) % (KT * C::DCH);
    const int r = idx / C::DCH, cc = idx % C::DCH;
    krow[i] = r;
    kcol[i] = (uint32_t)(cc * 8);
    ldsk[i] = (uint32_t)(r * C::KS + cc * 8);
    ldsv[i] = (uint32_t)(C::K_ELEMS + ((cc >> 2) * KT + r) * 32 + (cc & 3) * 8);
  }
  const int ldk32 = (int)ldk, ldv32 = (int)ldv;

  const int g16 = lane >> 4, i16 = lane & 15;
  // V^T tr-read lane offset inside a [32 d] image row block (elements)
  const int vtr = ((4 * hh + (i16 >> 2)) * 32) + 16 * (g16 & 1) + 4 * (i16 & 3);
  f32x16 oacc[C::NDB][QB];
  const bool bad = FIX || f32_loop<D, UNITC, false, QB>(lds, kb_ptr, vb_ptr, ldk32, ldv32, skv, krow, kcol, ldsk,
                                                           ldsv, qf, oacc, r32, hh, vtr, c);
  if (__syncthreads_or(bad)) {  // a score jumped > ~100 (log2) past mu somewhere: exact pass
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
      if (hh == C::MU_H) qf[qb][C::MU_KS][C::MU_J] = (__bf16)0.0f;
    f32_loop<D, UNITC, true, QB>(lds, kb_ptr, vb_ptr, ldk32, ldv32, skv, krow, kcol, ldsk, ldsv, qf, oacc, r32, hh,
                             vtr, c);
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l; register i of d-block db holds
  // d = 32*db + 8*(i>>2) + 4*hh + (i&3); swap 4-channel groups across lane halves
  // so each lane stores 8 consecutive channels (16 B).
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const float lown = oacc[C::L_DB][qb][C::L_I];
    const float lp = partner32(lown);
    const float l = hh == C::L_H ? lown : lp;
    const float inv = __builtin_amdgcn_rcpf(l);
    const int64_t qi = q0 + qb * 32 + r32;
    if (out_f32) {  // tests: O in fp32; register i of d-block db holds d = 32 db + 8 (i >> 2) + 4 hh + (i & 3)
      float* frow = (float*)o + (b * sq + qi) * ldo + (int64_t)h * D;
#pragma unroll
      for (int db = 0; db < C::NDB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d0 = 32 * db + 8 * g + 4 * hh;
          const f32x16& a = oacc[db][qb];
          if (qi < sq && d0 + 4 <= D)
            *(float4*)(frow + d0) = make_float4(a[4 * g] * inv, a[4 * g + 1] * inv, a[4 * g + 2] * inv, a[4 * g + 3] * inv);
        }
      continue;
    }
    bf16_t* orow = o + (b * sq + (qi < sq ? qi : 0)) * ldo + (int64_t)h * D;
#pragma unroll
    for (int db = 0; db < C::NDB; ++db) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const f32x16& a = oacc[db][qb];
        uint32_t x0 = pack2(a[8 * m + 0] * inv, a[8 * m + 1] * inv), x1 = pack2(a[8 * m + 2] * inv, a[8 * m + 3] * inv);
        uint32_t y0 = pack2(a[8 * m + 4] * inv, a[8 * m + 5] * inv), y1 = pack2(a[8 * m + 6] * inv, a[8 * m + 7] * inv);
        auto s0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
        auto s1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
        // lanes < 32: (x, y) = channels 16m + 0..7; lanes >= 32: channels 16m + 8..15
        const int dd = 32 * db + 16 * m + 8 * hh;
        if (qi < sq && dd + 8 <= D) *(uint4*)(orow + dd) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
      }
    }
  }
  };
  if constexpr (FIX) {
    __shared__ unsigned long long fmask;
    if (wave == 0) {
      const int64_t j = (int64_t)blockIdx.x * F32_FIXW + lane;
      const unsigned long long m = __ballot(lane < F32_FIXW && j < fix_blocks && flag_of(j));
      if (lane == 0) fmask = m;
    }
    __syncthreads();
    // workgroup-uniform: kept in SGPRs (a VGPR copy live across the exact pass spilled)
    const unsigned long long fm = fmask;
    unsigned long long m = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(fm >> 32)) << 32) |
                           __builtin_amdgcn_readfirstlane((uint32_t)fm);
    while (m) {
      const int bit = __builtin_ctzll(m);
      m &= m - 1;
      block((int)((int64_t)blockIdx.x * F32_FIXW + bit));
      __syncthreads();  // the next block rewrites the LDS tiles and padding
    }
  } else {
    block(xcd_remap(blockIdx.x, gridDim.x));
  }
}

}  // namespace

int vdattn::launch_flash32(const Args& a, const Plan& p) {
  const dim3 grid((unsigned)p.grid);
  if (p.unitc) return launch(flash32_kernel<40, true>, grid, NT, a, (int64_t)0);
  return launch(flash32_kernel<40, false>, grid, NT, a, (int64_t)0);
}

// flash40's exact pass (FIX, QB = 1): the instances live here, with the rest of flash32.
int vdattn::launch_flash32_exact(const Args& a, const Plan& p) {
  const dim3 grid((unsigned)p.fix_grid);
  const int64_t nfix = (a.sq + 127) / 128 * a.heads * a.batch;  // its 128-query blocks, F32_FIXW per workgroup
  if (p.unitc) return launch(flash32_kernel<40, true, true, 1>, grid, NT, a, nfix);
  return launch(flash32_kernel<40, false, true, 1>, grid, NT, a, nfix);
}
