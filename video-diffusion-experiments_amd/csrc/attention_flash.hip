// flash_attn_kernel — spatial self-attention and text cross-attention of
// diffusers Attention/AttnProcessor2_0 (F.scaled_dot_product_attention,
// SURVEY.md §8a a6/a7), bf16 MFMA with fp32 online softmax.
//
//   S^T = K . Q^T   (v_mfma_f32_16x16x32_bf16, A = K rows from LDS, B = Q^T
//                    from registers): the accumulator leaves each lane with 4
//                    keys of ONE query, so the row max needs 2 lane swaps and
//                    the row sum stays lane-local until the end.
//   O^T += V^T . P^T: the S^T accumulators of key blocks (2s, 2s+1), packed to
//                    bf16, ARE the P^T B-operand of k-step s (k order permuted;
//                    cdna_hip_programming.md §3 "accumulator as next operand"),
//                    and V^T comes out of LDS with ds_read_b64_tr_b16 (T10) in
//                    the same permuted key order.  No LDS round trip for P.
// Softmax VALU per score kept minimal: the scale is folded into the exp2
// argument (one FMA), the row max crosses lanes with v_permlane32/16_swap, the
// O rescale is skipped when no row max moved (wave-uniform), only a ragged
// last key tile is masked, and when PV is padded (d = 40 -> 48) column d of V
// holds 1.0 so the PV MFMA also produces the softmax row sum.
// Workgroup: 4 waves x 16*QBLK queries (QBLK = 4 for long sequences); K/V
// tiles of 64 keys double-buffered in LDS with the next tile's global loads
// issued before the current tile's MFMAs (T14).  Row strides are padded so
// 16-B K-row reads and the transposed V reads are bank-conflict free (§2/T10).
#include "attention_common.h"

namespace {

template <int D>
struct AttnCfg {
  static constexpr int DQK = (D + 31) / 32 * 32;          // QK^T contraction, padded
  static constexpr int DV = (D + 15) / 16 * 16;           // PV output columns, padded
  static constexpr int KS = DQK + 16;                     // K LDS row (elements): +32 B pad, conflict-free
                                                          // b128 fragment reads (tools/lds_banks.py)
  static constexpr int VS = ((DV * 2 + 31) / 64 * 64 + 32) / 2;  // V LDS row: 32B * odd
  static constexpr int KCH = DQK / 8;                     // K 16-byte chunks per row
  static constexpr int VCH = DV / 8;
  static constexpr int DCH = D / 8;                       // valid 16-byte chunks per K/V row
  static constexpr int LREG = (KT * DCH + NT - 1) / NT;   // staged K (and V) chunks per thread
};

template <int L>
__device__ __forceinline__ void kv_store(const stage_t<L>& st, bf16_t* kl, bf16_t* vl,
                                         const uint32_t (&ldsk)[L], const uint32_t (&ldsv)[L]) {
#pragma unroll
  for (int i = 0; i < L; ++i) {
    *(uint4*)(kl + ldsk[i]) = make_uint4(st[4 * i], st[4 * i + 1], st[4 * i + 2], st[4 * i + 3]);
    *(uint4*)(vl + ldsv[i]) = make_uint4(st[4 * L + 4 * i], st[4 * L + 4 * i + 1], st[4 * L + 4 * i + 2],
                                         st[4 * L + 4 * i + 3]);
  }
}

// CAUSAL (compile time; the CLIP text encoder's self-attention, sq == skv): query i sees keys
// j <= i.  A workgroup stops at the key tile that holds its last query (tiles wholly above the
// diagonal are never loaded; the bound is workgroup-uniform because staging is cooperative), and
// a wave masks the scores with key > query on the tiles that cross its diagonal.
//
// TAIL (compile time; VD_ATTN_TAIL, the IP-Adapter image tokens): the last `tail` (1..KT) of the
// skv K/V rows are a second segment with a softmax of its own,
//     o = softmax(q K_A^T) V_A + softmax(q K_B^T) V_B,   A = rows [0, skv - tail), B = the rest.
// Segment A runs the tile loop exactly as a call with skv - tail keys would (same tiles, same
// ragged mask, same clamped rows), then the accumulator is normalised in place by A's row sum —
// the epilogue's reciprocal and multiply, so with V_B = 0 the stored bits are those of the
// untailed call.  Segment B is one more trip through the loop on a single key tile loaded from
// row skv - tail (staged under A's last tile like any other): its softmax is exact in one pass
// (row max, p = exp2(s c - m), row sum across the query's 4 lanes, p / l packed to bf16) and its
// PV MFMAs accumulate onto the normalised A result in the same registers; the epilogue stores
// without dividing.  The ones column (DV > D) is spent once A is normalised, so B's row sum is
// always summed explicitly.
template <int D, int QBLK, bool CAUSAL = false, bool TAIL = false>
__global__ __launch_bounds__(NT, 2) void flash_attn_kernel(
    const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
    const bf16_t* __restrict__ v, int64_t ldv, bf16_t* __restrict__ o, int64_t ldo, int heads,
    int64_t sq, int64_t skv, int64_t kv_div, float c, int out_f32 = 0, int tail = 0) {
  static_assert(!(CAUSAL && TAIL), "a tailed call is never causal");
  using C = AttnCfg<D>;
  // When PV is padded (DV > D) column D of V is set to 1.0, so the PV MFMA also
  // produces the softmax row sum (no per-score adds).
  constexpr bool ONES = C::DV > D;
  constexpr int QWV = 16 * QBLK;  // queries per wave
  __shared__ __attribute__((aligned(16))) bf16_t ks_lds[2][KT * C::KS];
  __shared__ __attribute__((aligned(16))) bf16_t vs_lds[2][KT * C::VS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int64_t q0 = (int64_t)blockIdx.x * (4 * QWV) + wave * QWV;
  const int64_t bkv = b / kv_div;
  const bf16_t* qb_ptr = q + b * sq * ldq + (int64_t)h * D;
  const bf16_t* kb_ptr = k + bkv * skv * ldk + (int64_t)h * D;
  const bf16_t* vb_ptr = v + bkv * skv * ldv + (int64_t)h * D;
  const int fr = lane & 15, fg = lane >> 4;

  // Q^T fragments (B operand): lane holds Q[q0 + qb*16 + fr][dc*32 + 8*fg .. +7].
  bf16x8 qf[QBLK][C::DQK / 32];
#pragma unroll
  for (int qb = 0; qb < QBLK; ++qb) {
    const int64_t qi = q0 + qb * 16 + fr;
#pragma unroll
    for (int dc = 0; dc < C::DQK / 32; ++dc) {
      const int dd = dc * 32 + 8 * fg;
      uint4 u = make_uint4(0, 0, 0, 0);
      if (qi < sq && dd < D) u = *(const uint4*)(qb_ptr + qi * ldq + dd);
      qf[qb][dc] = __builtin_bit_cast(bf16x8, u);
    }
  }

  // K/V tile staging: only the D/8 valid chunks of each row are loaded; the
  // padding columns of both LDS buffers (zeros for K and V, and the 1.0 column
  // of V when ONES) are written once here and never overwritten.  Per-thread
  // (row, chunk) slots and their offsets are fixed for the whole kernel, so the
  // per-tile cost is one add per load; bounds are checked only on a ragged last tile.
  for (int idx = tid; idx < 2 * KT; idx += NT) {
    const int buf = idx / KT, r = idx % KT;
    for (int cc = C::DCH; cc < C::KCH; ++cc)
      *(uint4*)(&ks_lds[buf][r * C::KS + cc * 8]) = make_uint4(0, 0, 0, 0);
    for (int cc = C::DCH; cc < C::VCH; ++cc)
      *(uint4*)(&vs_lds[buf][r * C::VS + cc * 8]) = make_uint4(ONES && cc == C::DCH ? 0x3F80u : 0u, 0, 0, 0);
  }
  // Branch-free staging: every thread loads LREG (row, chunk) slots per tile;
  // slots past the tile's valid chunk count duplicate a valid one (same bytes to
  // the same LDS address), and rows past the last key are clamped to it (their
  // scores are masked to -inf, so P = 0 multiplies finite V).
  int krow[C::LREG];
  uint32_t kcol[C::LREG], ldsk[C::LREG], ldsv[C::LREG];
#pragma unroll
  for (int i = 0; i < C::LREG; ++i) {
    const int idx = (tid + i * NT) % (KT * C::DCH);
    const int r = idx / C::DCH, cc = idx % C::DCH;
    krow[i] = r;
    kcol[i] = (uint32_t)(cc * 8);
    ldsk[i] = (uint32_t)(r * C::KS + cc * 8);
    ldsv[i] = (uint32_t)(r * C::VS + cc * 8);
  }
  const int ldk32 = (int)ldk, ldv32 = (int)ldv;
  stage_t<C::LREG> kvst;

  f32x4 oacc[C::DV / 16][QBLK];
#pragma unroll
  for (int a = 0; a < C::DV / 16; ++a)
#pragma unroll
    for (int qb = 0; qb < QBLK; ++qb) oacc[a][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrow[QBLK], lrow[QBLK];  // running max (scaled, log2 units) / lane-partial row sum
#pragma unroll
  for (int qb = 0; qb < QBLK; ++qb) { mrow[qb] = -INFINITY; lrow[qb] = 0.f; }

  const int64_t kend = TAIL ? skv - tail : skv;  // keys of the tile loop (segment A of a tailed call)
  int ntiles = (int)((kend + KT - 1) / KT);
  if constexpr (CAUSAL) {  // stop at the tile of the workgroup's last query (blockIdx only: uniform)
    int64_t qlast = ((int64_t)blockIdx.x + 1) * (4 * QWV) - 1;
    if (qlast > sq - 1) qlast = sq - 1;
    const int nt = (int)(qlast / KT) + 1;
    if (nt < ntiles) ntiles = nt;
  }
  const bool ragged = (kend % KT) != 0;
  kvst = kv_load<C::LREG>(kb_ptr, vb_ptr, ldk32, ldv32, 0, kend, krow, kcol);
  kv_store<C::LREG>(kvst, ks_lds[0], vs_lds[0], ldsk, ldsv);
  __syncthreads();
  const int qq = fr >> 2, pp = fr & 3;  // tr-read geometry: lane 4*qq+pp -> row qq, cols 4*pp..

  // The two MFMA passes of a key tile for segment B's tile: the tile loop's own, restated.  The
  // loop keeps them inline — calling these helpers from it moved the untailed instances'
  // register allocation and schedule, 0.3 % of the flagship step in an A/B against the parent.
  // ---- S^T = K . Q^T
  auto qk_tile = [&](const bf16_t* kl, f32x4 (&s)[4][QBLK]) __attribute__((always_inline)) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int qb = 0; qb < QBLK; ++qb) s[kb][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    {  // K fragments two ahead in a rolling window (round 2): hipcc otherwise read each one right
       // before its QBLK MFMAs behind an lgkmcnt(0) — an exposed LDS latency per fragment
      constexpr int NK = C::DQK / 32 * 4;  // fragment i = (dc, kb) = (i / 4, i % 4)
      auto kfrag = [&](int i) { return *(const bf16x8*)(kl + ((i % 4) * 16 + fr) * C::KS + (i / 4) * 32 + 8 * fg); };
      bf16x8 k0 = kfrag(0), k1 = kfrag(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NK; ++i) {
        bf16x8 kn = k1;
        if (i + 2 < NK) kn = kfrag(i + 2);
#pragma unroll
        for (int qb = 0; qb < QBLK; ++qb)
          s[i % 4][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[qb][i / 4], s[i % 4][qb], 0, 0, 0);
        k0 = k1;
        k1 = kn;
      }
#pragma unroll
      for (int i = 0; i < NK; ++i) {
        if (i + 2 < NK) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, QBLK, 0);
      }
    }
  };
  // ---- O^T += V^T . P^T
  auto pv_tile = [&](const bf16_t* vl, const bf16x8 (&pf)[2][QBLK]) __attribute__((always_inline)) {
    {  // V^T fragments two ahead in a rolling window, as K above (fragment j = (a, st) = (j / 2, j % 2))
      constexpr int NV = C::DV / 16 * 2;
      auto vfrag = [&](int j) {
        const bf16_t* p0 = vl + (32 * (j % 2) + 4 * fg + qq) * C::VS + (j / 2) * 16 + 4 * pp;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(p0));
        const bf16x4 hi =
            __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(p0 + 16 * C::VS));
        return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      };
      bf16x8 v0 = vfrag(0), v1 = vfrag(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        bf16x8 vn = v1;
        if (j + 2 < NV) vn = vfrag(j + 2);
#pragma unroll
        for (int qb = 0; qb < QBLK; ++qb)
          oacc[j / 2][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, pf[j % 2][qb], oacc[j / 2][qb], 0, 0, 0);
        v0 = v1;
        v1 = vn;
      }
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if (j + 2 < NV) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, QBLK, 0);
      }
    }
  };

  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntiles) kvst = kv_load<C::LREG>(kb_ptr, vb_ptr, ldk32, ldv32, t + 1, kend, krow, kcol);
    if constexpr (TAIL) {  // segment B's one tile is staged under A's last, as every other tile is
      if (t + 1 == ntiles) kvst = kv_load_rows<C::LREG>(kb_ptr, vb_ptr, ldk32, ldv32, kend, tail - 1, krow, kcol);
    }
    const bf16_t* kl = ks_lds[buf];
    const bf16_t* vl = vs_lds[buf];

    // ---- S^T = K . Q^T
    f32x4 s[4][QBLK];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int qb = 0; qb < QBLK; ++qb) s[kb][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    {  // K fragments two ahead in a rolling window (round 2): hipcc otherwise read each one right
       // before its QBLK MFMAs behind an lgkmcnt(0) — an exposed LDS latency per fragment
      constexpr int NK = C::DQK / 32 * 4;  // fragment i = (dc, kb) = (i / 4, i % 4)
      auto kfrag = [&](int i) { return *(const bf16x8*)(kl + ((i % 4) * 16 + fr) * C::KS + (i / 4) * 32 + 8 * fg); };
      bf16x8 k0 = kfrag(0), k1 = kfrag(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NK; ++i) {
        bf16x8 kn = k1;
        if (i + 2 < NK) kn = kfrag(i + 2);
#pragma unroll
        for (int qb = 0; qb < QBLK; ++qb)
          s[i % 4][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[qb][i / 4], s[i % 4][qb], 0, 0, 0);
        k0 = k1;
        k1 = kn;
      }
#pragma unroll
      for (int i = 0; i < NK; ++i) {
        if (i + 2 < NK) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, QBLK, 0);
      }
    }
    if (ragged && t == ntiles - 1) {  // only the last tile of a ragged key range is masked
      const int64_t kbase = (int64_t)t * KT + 4 * fg;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (kbase + kb * 16 + j >= kend) {
#pragma unroll
            for (int qb = 0; qb < QBLK; ++qb) s[kb][qb][j] = -INFINITY;
          }
    }
    if constexpr (CAUSAL) {
      // Wave-uniform test: the tile's last key lies above the wave's first query.  Tile 0 is
      // always processed first and holds key 0 <= every query, so mrow is finite before any tile
      // that is fully masked for this wave; there mx = -inf, mnew = mrow, p = 0, alpha = 1 and no
      // exp2(-inf - -inf) can occur (c > 0 is checked by attention_entry).
      if ((int64_t)t * KT + (KT - 1) > q0) {
        const int64_t kbase = (int64_t)t * KT + 4 * fg;
#pragma unroll
        for (int qb = 0; qb < QBLK; ++qb) {
          const int64_t qi = q0 + qb * 16 + fr;
#pragma unroll
          for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (kbase + kb * 16 + j > qi) s[kb][qb][j] = -INFINITY;
        }
      }
    }
    // ---- online softmax in log2 units: p = exp2(s*c - m)
    bf16x8 pf[2][QBLK];
    bool any_rescale = false;
    float alpha[QBLK];
#pragma unroll
    for (int qb = 0; qb < QBLK; ++qb) {
      float mx = s[0][qb][0];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) mx = fmaxf(mx, s[kb][qb][j]);
      mx = max_over_query_lanes(mx) * c;
      const float mnew = fmaxf(mrow[qb], mx);
      alpha[qb] = __builtin_amdgcn_exp2f(mrow[qb] - mnew);
      any_rescale |= mnew != mrow[qb];
      mrow[qb] = mnew;
      float ls = 0.f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[kb][qb][j], c, -mnew));
          s[kb][qb][j] = p;
          if (!ONES) ls += p;
        }
      if (!ONES) lrow[qb] = lrow[qb] * alpha[qb] + ls;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        bf16x8 f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f[j] = (__bf16)s[2 * st][qb][j];
          f[4 + j] = (__bf16)s[2 * st + 1][qb][j];
        }
        pf[st][qb] = f;
      }
    }
    if (__any(any_rescale)) {  // wave-uniform: skip the O-wide multiply when no max moved
#pragma unroll
      for (int a = 0; a < C::DV / 16; ++a)
#pragma unroll
        for (int qb = 0; qb < QBLK; ++qb)
#pragma unroll
          for (int j = 0; j < 4; ++j) oacc[a][qb][j] *= alpha[qb];
    }
    // ---- O^T += V^T . P^T
    {  // V^T fragments two ahead in a rolling window, as K above (fragment j = (a, st) = (j / 2, j % 2))
      constexpr int NV = C::DV / 16 * 2;
      auto vfrag = [&](int j) {
        const bf16_t* p0 = vl + (32 * (j % 2) + 4 * fg + qq) * C::VS + (j / 2) * 16 + 4 * pp;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(p0));
        const bf16x4 hi =
            __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(p0 + 16 * C::VS));
        return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      };
      bf16x8 v0 = vfrag(0), v1 = vfrag(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        bf16x8 vn = v1;
        if (j + 2 < NV) vn = vfrag(j + 2);
#pragma unroll
        for (int qb = 0; qb < QBLK; ++qb)
          oacc[j / 2][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, pf[j % 2][qb], oacc[j / 2][qb], 0, 0, 0);
        v0 = v1;
        v1 = vn;
      }
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if (j + 2 < NV) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, QBLK, 0);
      }
    }
    if (t + 1 < ntiles + (TAIL ? 1 : 0)) kv_store<C::LREG>(kvst, ks_lds[buf ^ 1], vs_lds[buf ^ 1], ldsk, ldsv);
    __syncthreads();
  }
  if constexpr (TAIL) {
    // ---- segment B (peeled: the running max and sum, the rescale factors and the staging
    // registers are dead here; as a run-time branch inside the loop it cost 20-60 VGPRs and
    // spilled the QBLK 4 instances).  It holds `tail` keys; the rest of its tile are clamped
    // duplicates and masked.
    const int buf = ntiles & 1;
    f32x4 s[4][QBLK];
    qk_tile(ks_lds[buf], s);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * fg + kb * 16 + j >= tail) {
#pragma unroll
          for (int qb = 0; qb < QBLK; ++qb) s[kb][qb][j] = -INFINITY;
        }
    // segment A is complete: O /= l, the epilogue's arithmetic
#pragma unroll
    for (int qb = 0; qb < QBLK; ++qb) {
      float l;
      if constexpr (ONES) {
        constexpr int a1 = D / 16, r1 = D % 16;
        l = __shfl(oacc[a1][qb][r1 % 4], (r1 / 4) * 16 + fr, 64);
      } else {
        l = lrow[qb];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
      }
      const float inv = 1.0f / l;
#pragma unroll
      for (int a = 0; a < C::DV / 16; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) oacc[a][qb][j] *= inv;
    }
    // one-pass softmax of segment B: P = exp2(s*c - m) / l
    bf16x8 pf[2][QBLK];
#pragma unroll
    for (int qb = 0; qb < QBLK; ++qb) {
      float mx = s[0][qb][0];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) mx = fmaxf(mx, s[kb][qb][j]);
      mx = max_over_query_lanes(mx) * c;  // finite: key 0 of the segment is never masked
      float ls = 0.f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[kb][qb][j], c, -mx));
          s[kb][qb][j] = p;
          ls += p;
        }
      ls += __shfl_xor(ls, 16, 64);
      ls += __shfl_xor(ls, 32, 64);
      const float inv = 1.0f / ls;  // ls >= 1: the row max contributes exp2(0)
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        bf16x8 f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f[j] = (__bf16)(s[2 * st][qb][j] * inv);
          f[4 + j] = (__bf16)(s[2 * st + 1][qb][j] * inv);
        }
        pf[st][qb] = f;
      }
    }
    pv_tile(vs_lds[buf], pf);
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l (a tailed call normalised each segment already)
#pragma unroll
  for (int qb = 0; qb < QBLK; ++qb) {
    float inv = 1.0f;
    if constexpr (!TAIL) {
      float l;
      if constexpr (ONES) {
        constexpr int a1 = D / 16, r1 = D % 16;
        l = __shfl(oacc[a1][qb][r1 % 4], (r1 / 4) * 16 + fr, 64);
      } else {
        l = lrow[qb];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
      }
      inv = 1.0f / l;
    }
    const int64_t qi = q0 + qb * 16 + fr;
    if (qi >= sq) continue;
    bf16_t* orow = o + (b * sq + qi) * ldo + (int64_t)h * D;
    float* frow = (float*)o + (b * sq + qi) * ldo + (int64_t)h * D;  // out_f32: O in fp32 (tests)
#pragma unroll
    for (int a = 0; a < C::DV / 16; ++a) {
      const int dd = a * 16 + 4 * fg;
      if (dd < D) {
        if (out_f32)
          *(float4*)(frow + dd) = make_float4(oacc[a][qb][0] * inv, oacc[a][qb][1] * inv, oacc[a][qb][2] * inv,
                                              oacc[a][qb][3] * inv);
        else
          *(uint2*)(orow + dd) = make_uint2(pack2(oacc[a][qb][0] * inv, oacc[a][qb][1] * inv),
                                            pack2(oacc[a][qb][2] * inv, oacc[a][qb][3] * inv));
      }
    }
  }
}

// QBLK 4 is instantiated for D <= 40 only: wider heads' QBLK-4 instances spill 94-280 VGPRs.
template <int D, bool CAUSAL, bool TAIL>
int launch_d(const vdattn::Args& a, const vdattn::Plan& p) {
  // p.grid = (64 QBLK)-query blocks x heads x batch
  const dim3 grid((unsigned)(p.grid / ((int64_t)a.heads * a.batch)), (unsigned)a.heads, (unsigned)a.batch);
  if constexpr (D <= 40) {
    if (p.qblk == 4) return vdattn::launch(flash_attn_kernel<D, 4, CAUSAL, TAIL>, grid, NT, a, p.tail);
  }
  return vdattn::launch(flash_attn_kernel<D, 2, CAUSAL, TAIL>, grid, NT, a, p.tail);
}

}  // namespace

// The instance set: plain for every d, causal for d = 32 / 64 (CLIP), tailed for the widths of the
// UNet's cross-attention (IP-Adapter).  plan() refuses every other combination before this.
int vdattn::launch_flash(int d, const Args& a, const Plan& p) {
  if (p.tail) {
    switch (d) {
      case 32: return launch_d<32, false, true>(a, p);
      case 40: return launch_d<40, false, true>(a, p);
      case 64: return launch_d<64, false, true>(a, p);
      case 80: return launch_d<80, false, true>(a, p);
      case 160: return launch_d<160, false, true>(a, p);
    }
  } else if (p.causal) {
    switch (d) {
      case 32: return launch_d<32, true, false>(a, p);
      case 64: return launch_d<64, true, false>(a, p);
    }
  } else {
    switch (d) {
      case 32: return launch_d<32, false, false>(a, p);
      case 40: return launch_d<40, false, false>(a, p);
      case 64: return launch_d<64, false, false>(a, p);
      case 80: return launch_d<80, false, false>(a, p);
      case 128: return launch_d<128, false, false>(a, p);
      case 160: return launch_d<160, false, false>(a, p);
    }
  }
  return VD_EUNSUPPORTED;
}
