// ============================================================================ v5
// Persistent 256 x 320 GEMM / implicit-GEMM conv, BK = 32, 8 waves as 4(M) x 2(N)
// (64 x 160 per wave: 4 x 10 accumulators of 16x16), 4-stage LDS-DMA ring (36 KiB per
// stage, three k-steps in flight), persistent strided unit walk as v2.  320 divides
// every N of the UNet (320 ... 10240): no padding.  One raw s_barrier per k-step behind
// a counted vmcnt; the DMA for k-step it+3 goes out right after the barrier of k-step
// it into the stage read at it-1.  Load-free epilogue (epi_fast) where it applies: the
// stores stay in flight across the next k-steps' counted waits.
// Measured against v2/v3 (tools/kbench.py): wins on the L1 attention QKV
// projection (M 131072, K 320, N 960: 145 vs 169 us), ties or loses elsewhere — the
// k-loop is bound by LDS-read / MFMA phase lock of the two waves on each SIMD and by
// the DMA of 64-B row segments, which neither two workgroups per CU, a dedicated
// L2-prefetch wave nor a two-group ping-pong schedule (all built and measured this
// round) removed.
// LDS operand image: rows of 64 B (4 chunks of 16 B); logical chunk c of row r
// sits in physical chunk c ^ ((r >> 2) & 2), which makes the 16x16x32 fragment
// reads (ds_read_b128: 16-lane groups over rows 0-3/12-15 and 4-11) conflict
// free.  The permutation is applied to the per-lane DMA SOURCE address, the
// image stays lane-linear (cdna_hip_programming.md rule 21).
#include "gemm_common.h"

namespace {

template <int BN, int WM, int WN, int STAGES>
struct G4 {
  static constexpr int NT = WM * WN * 64;
  static constexpr int NW = WM * WN;
  static constexpr int A_BYTES = G4_BM * G4_BK * 2;  // 16 KiB
  static constexpr int B_BYTES = BN * G4_BK * 2;
  static constexpr int STAGE = A_BYTES + B_BYTES;
  static constexpr int NPA = G4_BM / 16;             // A DMA pieces (16 rows x 64 B = 1 KiB) per k-step
  static constexpr int NPB = BN / 16;                // W DMA pieces per k-step
  // wave w issues A pieces w + NW*j (j < NAMAX) and W pieces w + NW*j (j < NBMAX)
  static constexpr int NAMAX = (NPA + NW - 1) / NW;
  static constexpr int NBMAX = (NPB + NW - 1) / NW;
  static constexpr int WROWS = G4_BM / WM, WCOLS = BN / WN;
  static constexpr int MB = WROWS / 16, NB = WCOLS / 16;
  // a ring of 4 per-unit bias slots (2 KiB each: two 1-KiB DMA pieces) for epi_fast
  static constexpr int BIAS_SLOTS = 4;
  static constexpr int LDS_BYTES = STAGES * STAGE + BIAS_SLOTS * 2048;
  static_assert(BN % (16 * WN) == 0 && G4_BM % (16 * WM) == 0, "tile / wave grid mismatch");
};

__device__ __forceinline__ uint32_t g4_off(int row, int chunk) {  // byte offset in an operand image
  return (uint32_t)(row * 64 + ((chunk ^ ((row >> 2) & 2)) << 4));
}

// Epilogue with the next LayerNorm fused (vd_gemm_desc.ln_out; v5 with N == BN == 320, so
// the workgroup's tile owns whole rows): x = bf16(acc + bias (+ res)) is stored as usual and
// kept in registers; row sums of the rounded x (lane: 4 columns x NB blocks; then the 4 lanes
// of a row by xor shuffles; then the WN = 2 column waves through `red` in LDS), mean, the
// two-pass variance the same way, and ln_out = fmaf((x - mean) * rstd, gamma, beta) (+ pe)
// — vd_layernorm's arithmetic on the same bf16 x (only the fp32 summation order differs).
// Every wave of the workgroup runs it (two s_barriers).
template <int MB, int NB>
__device__ __forceinline__ void epi_ln(const vd_gemm_desc& d, f32x4 (&acc)[NB][MB], int mbase, int nbase, int lane,
                                       int rloc, int wn, float* red) {
  static_assert(NB % 2 == 0, "epi_ln: whole 16-column pairs");
  const int M = (int)d.M, N = (int)d.N;
  const int fr = lane & 15, fq = lane >> 4;
  const int wcol = 16 * (fq & 1) + 8 * (fq >> 1);  // lane's first column inside a swapped pair
  bf16_t* out = (bf16_t*)d.out;
  // x: v_permlane16_swap of blocks (a, a+1) leaves each lane 8 consecutive columns of its row
  // (16-B residual loads and stores, as gemm_epilogue's wide path); the rounded x stays in acc
  // in that swapped order (a row's statistics do not depend on it)
#pragma unroll
  for (int a = 0; a < NB; a += 2) {
    const int n = nbase + a * 16 + wcol;
    float bv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (d.bias) {
      const float4 t0 = *(const float4*)(d.bias + n), t1 = *(const float4*)(d.bias + n + 4);
      bv[0] = t0.x; bv[1] = t0.y; bv[2] = t0.z; bv[3] = t0.w;
      bv[4] = t1.x; bv[5] = t1.y; bv[6] = t1.z; bv[7] = t1.w;
    }
    // the MB residual rows of this column pair load together, ahead of the stores below (round 2):
    // hipcc cannot move a residual load above an earlier `out` store (they may alias), so one
    // load per row interleaved with the stores made MB dependent HBM round trips per pair
    // (fused LN + residual at L1: 119 -> 110 us; gamma / beta staged in LDS as well spilled)
    uint4 rsv[MB];
    if (d.res) {
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        const int m = mbase + b * 16 + fr;
        rsv[b] = *(const uint4*)((const bf16_t*)d.res + (uint32_t)((m < M ? m : 0) * (int)d.ld_res + n));
      }
    }
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      const int m = mbase + b * 16 + fr;
      const bool mok = m < M;
      const int mrow = mok ? m : 0;
      float o[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[a][b][j]), __float_as_uint(acc[a + 1][b][j]),
                                                  false, false);
        o[j] = __uint_as_float(r[0]) + bv[j];
        o[4 + j] = __uint_as_float(r[1]) + bv[4 + j];
      }
      if (d.res) {
        float rf[8];
        unpack8(rsv[b], rf);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += rf[j];
      }
      const uint4 pk = pack8(o);
      if (mok) *(uint4*)(out + (uint32_t)(mrow * (int)d.ldc + n)) = pk;
      float x8[8];
      unpack8(pk, x8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[a][b][j] = x8[j];
        acc[a + 1][b][j] = x8[4 + j];
      }
    }
  }
  float mean[MB], rstd[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    float sm = 0.f;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) sm += acc[a][b][j];
    sm += __shfl_xor(sm, 16, 64);
    sm += __shfl_xor(sm, 32, 64);
    mean[b] = sm;
    if (fq == 0) red[wn * 256 + rloc + b * 16 + fr] = sm;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int b = 0; b < MB; ++b) mean[b] = (mean[b] + red[(1 - wn) * 256 + rloc + b * 16 + fr]) / (float)N;
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    float s2 = 0.f;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = acc[a][b][j] - mean[b];
        s2 = fmaf(t, t, s2);
      }
    s2 += __shfl_xor(s2, 16, 64);
    s2 += __shfl_xor(s2, 32, 64);
    rstd[b] = s2;
    if (fq == 0) red[512 + wn * 256 + rloc + b * 16 + fr] = s2;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int b = 0; b < MB; ++b)
    rstd[b] = rsqrtf((rstd[b] + red[512 + (1 - wn) * 256 + rloc + b * 16 + fr]) / (float)N + d.ln_eps);
  bf16_t* y = (bf16_t*)d.ln_out;
  int perow[MB];  // element offset of row m's PE row (m clamped; unused without ln_pe)
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    const int m = mbase + b * 16 + fr;
    perow[b] = d.ln_pe ? ((m < M ? m : 0) / (int)d.ln_pe_div) % (int)d.ln_pe_period * N : 0;
  }
#pragma unroll
  for (int a = 0; a < NB; a += 2) {
    const int n = nbase + a * 16 + wcol;
    const float4 g0 = *(const float4*)(d.ln_gamma + n), g1 = *(const float4*)(d.ln_gamma + n + 4);
    const float4 b0 = *(const float4*)(d.ln_beta + n), b1 = *(const float4*)(d.ln_beta + n + 4);
    const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      const int m = mbase + b * 16 + fr;
      if (m >= M) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = fmaf((acc[a][b][j] - mean[b]) * rstd[b], gg[j], bb[j]);
        o[4 + j] = fmaf((acc[a + 1][b][j] - mean[b]) * rstd[b], gg[4 + j], bb[4 + j]);
      }
      if (d.ln_pe) {
        const float4 t0 = *(const float4*)(d.ln_pe + perow[b] + n), t1 = *(const float4*)(d.ln_pe + perow[b] + n + 4);
        o[0] += t0.x; o[1] += t0.y; o[2] += t0.z; o[3] += t0.w;
        o[4] += t1.x; o[5] += t1.y; o[6] += t1.z; o[7] += t1.w;
      }
      *(uint4*)(y + (uint32_t)(m * (int)d.ld_ln + n)) = pack8(o);
    }
  }
}

template <int BN, int WM, int WN, int STAGES, int MODE, bool LN = false>
__global__ __attribute__((amdgpu_flat_work_group_size(1, WM * WN * 64), amdgpu_waves_per_eu(2))) void gemm4_kernel(
    const vd_gemm_desc d, uint32_t a0_bytes, uint32_t a1_bytes, uint32_t w_bytes, int split) {
  using C = G4<BN, WM, WN, STAGES>;
  __shared__ __attribute__((aligned(1024))) char smem[C::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int64_t M = d.M, N = d.N, K = d.K;
  const int tiles_n = (int)((N + BN - 1) / BN);
  const int tiles_m = (int)((M + G4_BM - 1) / G4_BM);
  const int units = tiles_n * tiles_m * split;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);  // see v2: XCD-contiguous strided walk
  const int G = gridDim.x;
  const int nk_all = (int)(K / G4_BK);

  const int rb = lane >> 2;                                               // row within the 16-row DMA piece
  const uint32_t lc16 = (uint32_t)(((lane & 3) ^ ((rb >> 2) & 2)) * 16);  // logical source chunk (bytes)
  const __amdgpu_buffer_rsrc_t ra0 = __builtin_amdgcn_make_buffer_rsrc((void*)d.a0, 0, a0_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ra1 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(d.a1 ? d.a1 : d.a0), 0, d.a1 ? a1_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)d.w, 0, w_bytes, 0x00020000);
  // this wave's pieces per k-step
  const int na_w = (C::NPA - wid + C::NW - 1) / C::NW;
  const int nb_w = (C::NPB - wid + C::NW - 1) / C::NW;
  const int per_step = na_w + nb_w;
  const int cin = mode_is_conv(MODE) ? (int)(K / 9) : 0;
  // pad-end: stride 2 and no upsample are the mode itself (checked by vd_gemm), so constants here
  const int cstride = MODE == A_CONV_PAD_END ? 2 : d.stride, cup = MODE == A_CONV_PAD_END ? 0 : d.upsample;
  const int hgrid = cup ? 2 * d.h_in : d.h_in;
  const int wgrid = cup ? 2 * d.w_in : d.w_in;
  // load-free epilogue (epi_fast) for plain bf16 outputs
  const bool fast = !LN && split == 1 && !d.res && !d.rowbias && !d.out_f32 && !d.rmap_inner && (N % 8) == 0 &&
                    (d.ldc % 8) == 0 && (((uintptr_t)d.out) & 15) == 0;
  const __amdgpu_buffer_rsrc_t rbias = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(d.bias ? d.bias : (const float*)d.a0), 0, d.bias ? (uint32_t)(N * 4) : 0u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rout =
      __builtin_amdgcn_make_buffer_rsrc(d.out, 0, (uint32_t)(M * d.ldc * 2), 0x00020000);
  int iun = 0, cun = 0;  // per-workgroup unit ordinals of the issue and compute cursors (bias slot)

  // ---- issue cursor: the (unit, k-step) whose DMA goes out next
  int iu = lid, ikt = 0, ikt1 = 0;
  uint32_t boff[C::NBMAX], aoff0[C::NAMAX], aoff1[C::NAMAX];
  // conv rows: base pixel of the row's image and its (oh, ow) packed 16:16
  int pimg[C::NAMAX], pohw[C::NAMAX];
  int c_tap = 0, c_ci = 0;
  bool c_new = true;
  // (an early-out for split == 1 here measured 15 % slower on the dense v2 GEMMs, same box,
  // profiles/r03t_unit_kr_bisect.txt: it changes how hipcc lays out the persistent unit loop)
  auto unit_kr = [&](int u, int& kt0, int& kt1) {
    const int sp = u % split;
    kt0 = (int)((int64_t)nk_all * sp / split);
    kt1 = (int)((int64_t)nk_all * (sp + 1) / split);
  };
  auto setup_unit = [&](int u) {
    const int tile = u / split;
    const int64_t m0 = (int64_t)(tile / tiles_n) * G4_BM, n0 = (int64_t)(tile % tiles_n) * BN;
    int kt0;
    unit_kr(u, kt0, ikt1);
    ikt = kt0;
#pragma unroll
    for (int j = 0; j < C::NBMAX; ++j) {
      int64_t n = n0 + (wid + C::NW * j) * 16 + rb;
      n = n < N ? n : N - 1;
      boff[j] = (uint32_t)(n * d.ldw * 2) + lc16;
    }
    if constexpr (MODE == VD_A_DENSE) {
#pragma unroll
      for (int j = 0; j < C::NAMAX; ++j) {
        int64_t m = m0 + (wid + C::NW * j) * 16 + rb;
        m = m < M ? m : M - 1;
        aoff0[j] = (uint32_t)(m * d.lda0 * 2) + lc16;
        aoff1[j] = (uint32_t)(m * d.lda1 * 2) + lc16;
      }
    } else {
      const int hw = d.h_out * d.w_out;
      const Div dhw(hw), dw(d.w_out);
#pragma unroll
      for (int j = 0; j < C::NAMAX; ++j) {
        int m = (int)m0 + (wid + C::NW * j) * 16 + rb;
        m = m < (int)M ? m : (int)M - 1;
        const int img = dhw(m);
        const int p = m - img * hw;
        const int oh = dw(p);
        pimg[j] = img * d.h_in * d.w_in;
        pohw[j] = (oh << 16) | (p - oh * d.w_out);
      }
      c_tap = kt0 * G4_BK / cin;
      c_ci = kt0 * G4_BK - c_tap * cin;
      c_new = true;
    }
  };
  auto issue = [&](int stage) {  // DMA of the cursor's k-step into `stage`, then advance the cursor
    char* la = smem + stage * C::STAGE;
    char* lb = la + C::A_BYTES;
    const int kb = ikt * G4_BK;
    {
      if (fast && wid == 0 && ikt == (int)((int64_t)nk_all * (iu % split) / split)) {
        // first k-step of a unit: its BN bias values (zeros past N or without bias) into slot iun & 3
        char* bs = smem + STAGES * C::STAGE + (iun & (C::BIAS_SLOTS - 1)) * 2048;
        const uint32_t nb0 = (uint32_t)((iu / split) % tiles_n) * BN * 4 + lane * 16;
        dma16(rbias, bs, nb0);
        dma16(rbias, bs + 1024, nb0 + 1024);
      }
      if constexpr (MODE == VD_A_DENSE) {
        const bool s0 = kb < (int)d.k0;
        const uint32_t koff = (uint32_t)(s0 ? kb : kb - (int)d.k0) * 2;
#pragma unroll
        for (int j = 0; j < C::NAMAX; ++j)
          if (j < na_w) dma16(s0 ? ra0 : ra1, la + (wid + C::NW * j) * 1024, (s0 ? aoff0[j] : aoff1[j]) + koff);
      } else {
        if (c_new) {  // new tap: recompute the rows' pixel offsets
          c_new = false;
          const int dy = c_tap / 3, dx = c_tap - 3 * dy;
#pragma unroll
          for (int j = 0; j < C::NAMAX; ++j) {
            int ih = (pohw[j] >> 16) * cstride + dy - conv_pad_lo<MODE>,
                iw = (pohw[j] & 0xffff) * cstride + dx - conv_pad_lo<MODE>;
            const bool ok = ((uint32_t)ih < (uint32_t)hgrid) & ((uint32_t)iw < (uint32_t)wgrid);  // branch-free
            ih >>= cup;
            iw >>= cup;
            const uint32_t pix = (uint32_t)(pimg[j] + ih * d.w_in + iw);
            aoff0[j] = ok ? pix * (uint32_t)(d.lda0 * 2) + lc16 : G2_OOB;
            aoff1[j] = ok ? pix * (uint32_t)(d.lda1 * 2) + lc16 : G2_OOB;
          }
        }
        const bool s0 = c_ci < (int)d.k0;
        const uint32_t coff = (uint32_t)(s0 ? c_ci : c_ci - (int)d.k0) * 2;
#pragma unroll
        for (int j = 0; j < C::NAMAX; ++j) {
          const uint32_t o = s0 ? aoff0[j] : aoff1[j];
          if (j < na_w) dma16(s0 ? ra0 : ra1, la + (wid + C::NW * j) * 1024, o + coff);
        }
      }
#pragma unroll
      for (int j = 0; j < C::NBMAX; ++j)
        if (j < nb_w) dma16(rw, lb + (wid + C::NW * j) * 1024, boff[j] + (uint32_t)kb * 2);
    }
    if constexpr (mode_is_conv(MODE)) {
      c_ci += G4_BK;
      if (c_ci == cin) { c_ci = 0; ++c_tap; c_new = true; }
    }
    if (++ikt == ikt1) {
      ++iun;
      if ((iu += G) < units) setup_unit(iu);
    }
  };

  f32x4 acc[C::NB][C::MB];
#pragma unroll
  for (int a = 0; a < C::NB; ++a)
#pragma unroll
    for (int b = 0; b < C::MB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  int n_it = 0;
  for (int u = lid; u < units; u += G) {
    int a0_, a1_;
    unit_kr(u, a0_, a1_);
    n_it += a1_ - a0_;
  }
  if (n_it == 0) return;
  setup_unit(lid);
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < n_it) issue(s);
  const int fr = lane & 15, fq = lane >> 4;
  const uint32_t wlane = C::A_BYTES + g4_off(wn * C::WCOLS + fr, fq);
  const uint32_t xlane = g4_off(wm * C::WROWS + fr, fq);
  int cu = lid, ckt, ckt1;
  unit_kr(cu, ckt, ckt1);
  int stage = 0;
  int st1 = 0, st2 = 0, st3 = 0;  // epilogue stores issued 1, 2, 3 iterations ago (still younger than k-step it's DMA)
  for (int it = 0; it < n_it; ++it) {
    // this wave's DMA for k-step `it` has landed once only the younger k-steps' (at
    // most S-2 of them) remain outstanding, plus the epilogue stores issued since
    // k-step it's DMA went out (iterations it-S+1 .. it-1); the barrier then publishes
    // every wave's part and certifies that stage (it-1)%S, the target of the next
    // issue, is no longer read.
    {
      const int younger = n_it - 1 - it < STAGES - 2 ? n_it - 1 - it : STAGES - 2;
      const int pend = st1 + (STAGES >= 3 ? st2 : 0) + (STAGES >= 4 ? st3 : 0);
      wait_vm_rt(younger * per_step + pend);
    }
    st3 = st2;
    st2 = st1;
    st1 = 0;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (it + STAGES - 1 < n_it) issue(stage == 0 ? STAGES - 1 : stage - 1);
    const char* sbase = smem + stage * C::STAGE;
    if constexpr (C::MB == 8) {
      // W once, X in two halves of 4 (caps the live fragment registers)
      bf16x8 wf[C::NB], xf[4];
#pragma unroll
      for (int a = 0; a < C::NB; ++a) wf[a] = *(const bf16x8*)(sbase + wlane + a * 1024);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int b = 0; b < 4; ++b) xf[b] = *(const bf16x8*)(sbase + xlane + (4 * h + b) * 1024);
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int a = 0; a < C::NB; ++a)
            acc[a][4 * h + b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a], xf[b], acc[a][4 * h + b], 0, 0, 0);
      }
    } else {
      // X once; W fragments two ahead in a rolling window (round 2): each W read issues under the
      // MFMAs of the fragment two before it, pinned by sched_group_barrier — the halves below let
      // hipcc wait lgkmcnt on every pair right before its MFMAs
      bf16x8 xf[C::MB];
#pragma unroll
      for (int b = 0; b < C::MB; ++b) xf[b] = *(const bf16x8*)(sbase + xlane + b * 1024);
      bf16x8 w0 = *(const bf16x8*)(sbase + wlane), w1 = *(const bf16x8*)(sbase + wlane + 1024);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int a = 0; a < C::NB; ++a) {
        bf16x8 wn = w1;
        if (a + 2 < C::NB) wn = *(const bf16x8*)(sbase + wlane + (a + 2) * 1024);
#pragma unroll
        for (int b = 0; b < C::MB; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, xf[b], acc[a][b], 0, 0, 0);
        w0 = w1;
        w1 = wn;
      }
#pragma unroll
      for (int a = 0; a < C::NB; ++a) {
        if (a + 2 < C::NB) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, C::MB, 0);
      }
    }
    if (++ckt == ckt1) {  // unit finished: epilogue
      const int tile = cu / split, sp = cu % split;
      const int64_t m0 = (int64_t)(tile / tiles_n) * G4_BM, n0 = (int64_t)(tile % tiles_n) * BN;
      bool done = false;
      if constexpr (LN) {  // plan: N == BN, split == 1; the bias slots (unused without `fast`) hold `red`
        static_assert(WN == 2 && C::BIAS_SLOTS * 2048 >= 4096, "epi_ln: two column waves, 4 KiB of LDS");
        epi_ln<C::MB, C::NB>(d, acc, (int)m0 + wm * C::WROWS, (int)n0 + wn * C::WCOLS, lane, wm * C::WROWS, wn,
                             (float*)(smem + STAGES * C::STAGE));
        done = true;
      } else if (fast) {
        const float* bsl = (const float*)(smem + STAGES * C::STAGE + (cun & (C::BIAS_SLOTS - 1)) * 2048);
        st1 = epi_fast<C::MB, C::NB>(d, acc, (int)m0 + wm * C::WROWS, (int)n0 + wn * C::WCOLS, lane, bsl,
                                     (int)n0, rout);
        done = true;
      }
      if (!LN && !done) {
        if (split == 1) {
          gemm_epilogue<C::MB, C::NB>(d, acc, (int)m0 + wm * C::WROWS, (int)n0 + wn * C::WCOLS, lane);
        } else {  // split-K: raw fp32 slab ws[sp][m][n]; gemm_splitk_reduce applies the epilogue
          float* slab = (float*)d.ws + (int64_t)sp * M * N;
#pragma unroll
          for (int a = 0; a < C::NB; ++a) {
            const int64_t n = n0 + wn * C::WCOLS + a * 16 + 4 * fq;
            if (n >= N) continue;
#pragma unroll
            for (int b = 0; b < C::MB; ++b) {
              const int64_t m = m0 + wm * C::WROWS + b * 16 + fr;
              if (m < M)
                *(float4*)(slab + m * N + n) = make_float4(acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]);
            }
          }
        }
      }
#pragma unroll
      for (int a = 0; a < C::NB; ++a)
#pragma unroll
        for (int b = 0; b < C::MB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      ++cun;
      if ((cu += G) < units) unit_kr(cu, ckt, ckt1);
    }
    stage = stage == STAGES - 1 ? 0 : stage + 1;
  }
}

}  // namespace

namespace vdgemm {

template <int BN, int WM, int WN, int STAGES>
static int launch4(const vd_gemm_desc& d, const Plan& p, hipStream_t s) {
  using C = G4<BN, WM, WN, STAGES>;
  const int64_t units = ((d.M + G4_BM - 1) / G4_BM) * ((d.N + BN - 1) / BN) * p.split;
  const dim3 grid((unsigned)persistent_grid(units));
  if (d.a_mode == VD_A_CONV3X3 && p.pad_end)
    hipLaunchKernelGGL((gemm4_kernel<BN, WM, WN, STAGES, A_CONV_PAD_END>), grid, dim3(C::NT), 0, s, d, p.a0b, p.a1b,
                       p.wb, p.split);
  else if (d.a_mode == VD_A_CONV3X3)
    hipLaunchKernelGGL((gemm4_kernel<BN, WM, WN, STAGES, VD_A_CONV3X3>), grid, dim3(C::NT), 0, s, d, p.a0b, p.a1b,
                       p.wb, p.split);
  else if (d.ln_out)  // the plan only lets a fusable descriptor keep ln_out
    hipLaunchKernelGGL((gemm4_kernel<BN, WM, WN, STAGES, VD_A_DENSE, true>), grid, dim3(C::NT), 0, s, d, p.a0b,
                       p.a1b, p.wb, p.split);
  else
    hipLaunchKernelGGL((gemm4_kernel<BN, WM, WN, STAGES, VD_A_DENSE>), grid, dim3(C::NT), 0, s, d, p.a0b, p.a1b,
                       p.wb, p.split);
  const int rc = vd_launch_status();
  return rc != VD_OK || p.split == 1 ? rc : launch_splitk_reduce(d, p.split, s);
}

int launch_v5(const vd_gemm_desc& d, const Plan& p, hipStream_t s) { return launch4<320, 4, 2, 4>(d, p, s); }

}  // namespace vdgemm
