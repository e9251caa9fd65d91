// ============================================================================ v2
// LDS-DMA GEMM: BM = 256, BN in {128, 160}, BK = 64, 512 threads = 8 waves as
// 4(M) x 2(N), each wave 64 x BN/2.  Operands reach LDS by `buffer_load_dwordx4
// ... lds` (no VGPR staging, no ds_write pass) into a 3-stage ring, two tiles in
// flight, ONE raw s_barrier per K-tile behind a counted vmcnt (guide §5
// "Pipelining across barriers").  The LDS image is lane-linear; the (row & 7)
// XOR swizzle is applied on the per-lane SOURCE address (rule 21).  Conv taps
// outside the image are zero-filled by the buffer range check (voffset beyond
// num_records returns 0).  Per-tile address work: one integer add per load.
#include "gemm_common.h"

namespace {

template <int BN>
struct G2 {
  static constexpr int A_BYTES = G2_BM * BK * 2;   // 32 KiB
  static constexpr int B_BYTES = BN * BK * 2;
  static constexpr int STAGE = A_BYTES + B_BYTES;
  static constexpr int NA = 4;                     // A DMA instructions per wave per tile
  static constexpr int NBI = BN / 8;               // B DMA instructions per tile (whole block)
  static constexpr int NBMAX = (NBI + 7) / 8;      // per wave, upper bound
  static constexpr int MB = 4, NB = BN / 32;
};

// Fragment-read order (round 2): without a pin hipcc sinks each X fragment read to its 4 MFMAs
// behind an lgkmcnt(0) — 8 exposed LDS latencies per K-tile.  k-step 0's 9 reads issue right
// after the barrier (sched_barrier), then k-step 1's reads interleave one per two of k-step 0's
// MFMAs (sched_group_barrier), so the MFMA chain waits on counted lgkmcnt only (52.79 vs 53.50
// ms/step for the unpinned order, 53.11 with all reads ahead; profiles/r02f_fragment_order.txt).

template <int BN, int MODE>
__global__ __launch_bounds__(G2_NT, 1) void gemm2_kernel(const vd_gemm_desc d, uint32_t a0_bytes,
                                                         uint32_t a1_bytes, uint32_t w_bytes,
                                                         int split) {
  using C = G2<BN>;
  __shared__ __attribute__((aligned(1024))) char smem[G2_STAGES * C::STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int64_t M = d.M, N = d.N, K = d.K;
  const int tiles_n = (int)((N + BN - 1) / BN);
  const int tiles_m = (int)((M + G2_BM - 1) / G2_BM);
  const int units = tiles_n * tiles_m * split;
  // Persistent, strided: this workgroup owns units lid, lid + G, lid + 2G, ...
  // (G = gridDim.x <= #CUs, all resident).  A unit is (output tile, split-K
  // slice), tiles N-fastest.  lid is XCD-contiguous (xcd_remap), so at every
  // round the ~32 workgroups of one XCD run ~32 CONSECUTIVE units — the N-tiles
  // of the same few A row-panels — and each A panel comes from HBM once and is
  // shared through that XCD's L2 (a contiguous per-workgroup range instead puts
  // 32 different panels in flight per XCD, thrashes L2 and re-reads A from HBM
  // once per N-tile).
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int G = gridDim.x;
  const int u_begin = lid;
  const int nk_all = (int)(K / BK);

  const int rb = lane >> 3;                                  // row within the 8-row DMA block
  const uint32_t lc16 = (uint32_t)(((lane & 7) ^ rb) * 16);  // swizzled source chunk (bytes)
  const __amdgpu_buffer_rsrc_t ra0 = __builtin_amdgcn_make_buffer_rsrc((void*)d.a0, 0, a0_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ra1 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(d.a1 ? d.a1 : d.a0), 0, d.a1 ? a1_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)d.w, 0, w_bytes, 0x00020000);
  const int nbw = (C::NBI - wid + 7) / 8;  // this wave's B DMA instructions per K-tile
  const int cin = mode_is_conv(MODE) ? (int)(K / (d.ks * d.ks * d.kt)) : 0;
  const int hgrid = d.upsample ? 2 * d.h_in : d.h_in;
  const int wgrid = d.upsample ? 2 * d.w_in : d.w_in;

  // ---- issue cursor: the (unit, k-tile) whose DMA goes out next
  int iu = u_begin, ikt = 0, ikt1 = 0;
  uint32_t boff[C::NBMAX], aoff0[C::NA], aoff1[C::NA];
  int poh[C::NA], pow_[C::NA], pimg[C::NA], pfr[C::NA];
  int c_tap = 0, c_ci = 0;
  bool c_new = true;
  // (an early-out for split == 1 here measured 15 % slower on the dense v2 GEMMs, same box,
  // profiles/r03t_unit_kr_bisect.txt: it changes how hipcc lays out the persistent unit loop)
  auto unit_kr = [&](int u, int& kt0, int& kt1) {
    const int sp = u % split;
    kt0 = (int)((int64_t)nk_all * sp / split);
    kt1 = (int)((int64_t)nk_all * (sp + 1) / split);
  };
  auto setup_unit = [&](int u) {  // per-unit row offsets for the issue cursor
    const int tile = u / split;
    const int64_t m0 = (int64_t)(tile / tiles_n) * G2_BM, n0 = (int64_t)(tile % tiles_n) * BN;
    int kt0;
    unit_kr(u, kt0, ikt1);
    ikt = kt0;
#pragma unroll
    for (int j = 0; j < C::NBMAX; ++j) {
      int64_t n = n0 + (j * 8 + wid) * 8 + rb;
      n = n < N ? n : N - 1;
      boff[j] = (uint32_t)(n * d.ldw * 2) + lc16;
    }
    if constexpr (MODE == VD_A_DENSE) {
#pragma unroll
      for (int j = 0; j < C::NA; ++j) {
        int64_t m = m0 + (wid * 4 + j) * 8 + rb;
        m = m < M ? m : M - 1;
        aoff0[j] = (uint32_t)(m * d.lda0 * 2) + lc16;
        aoff1[j] = (uint32_t)(m * d.lda1 * 2) + lc16;
      }
    } else {  // 32-bit rows, shifts for power-of-two sizes (round 3; int64 divisions: -2-3 %)
      const int hw = d.h_out * d.w_out;
      const Div dhw(hw), dfr(d.frames_out), dw(d.w_out);
#pragma unroll
      for (int j = 0; j < C::NA; ++j) {
        int m = (int)m0 + (wid * 4 + j) * 8 + rb;
        m = m < (int)M ? m : (int)M - 1;
        const int img = dhw(m);
        const int vid = dfr(img);
        pfr[j] = img - vid * d.frames_out + d.t_off - d.kt / 2;  // frame of temporal tap 0
        pimg[j] = vid * d.frames_in + pfr[j];
        const int p = m - img * hw;
        poh[j] = dw(p);
        pow_[j] = p - poh[j] * d.w_out;
      }
    }
    if constexpr (MODE != VD_A_DENSE) {
      c_tap = kt0 * BK / cin;
      c_ci = kt0 * BK - c_tap * cin;
      c_new = true;
    }
  };
  auto issue = [&](int stage) {  // DMA of the cursor's k-tile into `stage`, then advance it
    char* la = smem + stage * C::STAGE;
    char* lb = la + C::A_BYTES;
    const int kb = ikt * BK;
    if constexpr (MODE == VD_A_DENSE) {
      const bool s0 = kb < (int)d.k0;
      const uint32_t koff = (uint32_t)(s0 ? kb : kb - (int)d.k0) * 2;
#pragma unroll
      for (int j = 0; j < C::NA; ++j)
        dma16(s0 ? ra0 : ra1, la + (wid * 4 + j) * 1024, (s0 ? aoff0[j] : aoff1[j]) + koff);
    } else {
      if (c_new) {  // new tap: recompute the rows' pixel offsets
        c_new = false;
        const int ks2 = d.ks * d.ks;
        const int dt = c_tap / ks2, t9 = c_tap - ks2 * dt;
        const int dy = d.ks == 3 ? t9 / 3 : 1, dx = d.ks == 3 ? t9 - 3 * (t9 / 3) : 1;
        // branch-free (round 3): unsigned range checks combined with &, so hipcc emits no
        // exec-mask branches per row (the && chain compiled to three nested saveexec blocks)
#pragma unroll
        for (int j = 0; j < C::NA; ++j) {
          const int ih = poh[j] * d.stride + dy - conv_pad_lo<MODE>,
                    iw = pow_[j] * d.stride + dx - conv_pad_lo<MODE>;
          const int fin = pfr[j] + dt;
          const bool ok = ((uint32_t)ih < (uint32_t)hgrid) & ((uint32_t)iw < (uint32_t)wgrid) &
                          ((uint32_t)fin < (uint32_t)d.frames_in);
          const uint32_t pix = (uint32_t)(((pimg[j] + dt) * d.h_in + (ih >> d.upsample)) * d.w_in + (iw >> d.upsample));
          aoff0[j] = ok ? pix * (uint32_t)(d.lda0 * 2) + lc16 : G2_OOB;
          aoff1[j] = ok ? pix * (uint32_t)(d.lda1 * 2) + lc16 : G2_OOB;
        }
      }
      const bool s0 = c_ci < (int)d.k0;
      const uint32_t coff = (uint32_t)(s0 ? c_ci : c_ci - (int)d.k0) * 2;
      // a tap outside the image keeps G2_OOB + coff >= 2^31 > the buffer's num_records (< 2^31,
      // checked by plan()): still out of range, read as zeros — no per-piece select
#pragma unroll
      for (int j = 0; j < C::NA; ++j)
        dma16(s0 ? ra0 : ra1, la + (wid * 4 + j) * 1024, (s0 ? aoff0[j] : aoff1[j]) + coff);
      c_ci += BK;
      if (c_ci == cin) { c_ci = 0; ++c_tap; c_new = true; }
    }
#pragma unroll
    for (int j = 0; j < C::NBMAX; ++j)
      if (j < nbw) dma16(rw, lb + (j * 8 + wid) * 1024, boff[j] + (uint32_t)kb * 2);
    if (++ikt == ikt1 && (iu += G) < units) setup_unit(iu);
  };

  f32x4 acc[C::NB][C::MB];
#pragma unroll
  for (int a = 0; a < C::NB; ++a)
#pragma unroll
    for (int b = 0; b < C::MB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // total k-tiles this workgroup streams
  int n_it = 0;
  for (int u = u_begin; u < units; u += G) {
    int a0_, a1_;
    unit_kr(u, a0_, a1_);
    n_it += a1_ - a0_;
  }
  if (n_it == 0) return;
  setup_unit(u_begin);
  issue(0);
  if (n_it > 1) issue(1);
  // per-lane LDS byte offsets of the first fragment of each operand for k-step
  // ks (rows differ by multiples of 16 between fragments, so the (row & 7) XOR
  // swizzle is the same and fragment a/b adds a constant)
  // Column map (BN = 160, 5 blocks per wave): wave wn owns the 64 columns 64 wn .. 64 wn + 63 as
  // two 16-B-store pairs, and the odd block at 128 + 16 wn, so every bf16 store segment is 64-B
  // aligned (an 80-column wave tile put wave 1's pairs across 64-B granules and wrote 1.6x,
  // profiles/r03w_gemm_traffic.txt). Rows stay 16-multiples apart: the LDS XOR is unchanged.
  constexpr bool ODDMAP = (C::NB % 2) == 1 && C::NB > 1;
  const int wcb = ODDMAP ? wn * 16 * (C::NB - 1) : wn * (BN / 2);  // the wave's first column
  const int wodd = ODDMAP ? 32 * (C::NB - 1) + 16 * wn : wcb + 16 * (C::NB - 1);  // odd block's column
  uint32_t wlane[BK / 32], xlane[BK / 32], wlodd[BK / 32];
#pragma unroll
  for (int ks = 0; ks < BK / 32; ++ks) {
    wlane[ks] = C::A_BYTES + 2 * lds_off(wcb + (lane & 15), ks * 4 + (lane >> 4));
    wlodd[ks] = wlane[ks] + (uint32_t)(wodd - wcb) * BK * 2;
    xlane[ks] = 2 * lds_off(wm * 64 + (lane & 15), ks * 4 + (lane >> 4));
  }
  // ---- compute cursor
  int cu = u_begin, ckt, ckt1;
  unit_kr(cu, ckt, ckt1);
  const int fr = lane & 15, fq = lane >> 4;
  int stage = 0;
  for (int it = 0; it < n_it; ++it) {
    // this wave's DMA for k-tile `it` has landed once at most k-tile it+1's remain
    // outstanding (everything issued before that, epilogue stores included, is done)
    if (it + 1 < n_it) {
      if (nbw == C::NBMAX) wait_vm<C::NA + C::NBMAX>();
      else wait_vm<C::NA + C::NBMAX - 1>();
    } else {
      wait_vm<0>();
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's DMA for `it` landed; stage (it-1)%3 fully read
    const char* sbase = smem + stage * C::STAGE;
    {
      bf16x8 wf[BK / 32][C::NB], xf[BK / 32][C::MB];
#pragma unroll
      for (int ks = 0; ks < BK / 32; ++ks) {
#pragma unroll
        for (int b = 0; b < C::MB; ++b) xf[ks][b] = *(const bf16x8*)(sbase + xlane[ks] + b * 16 * BK * 2);
#pragma unroll
        for (int a = 0; a < C::NB; ++a)
          wf[ks][a] = *(const bf16x8*)(sbase + (a == C::NB - 1 ? wlodd[ks] : wlane[ks] + a * 16 * BK * 2));
        if (ks == 0) __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int ks = 0; ks < BK / 32; ++ks)
#pragma unroll
        for (int a = 0; a < C::NB; ++a)
#pragma unroll
          for (int b = 0; b < C::MB; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks][a], xf[ks][b], acc[a][b], 0, 0, 0);
      {  // k-step 1's reads one per two of k-step 0's MFMAs
        constexpr int NR = C::MB + C::NB, NM = 2 * C::MB * C::NB;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NM - 2 * NR, 0);
      }
    }
    if (++ckt == ckt1) {  // unit finished: epilogue (its memory ops precede the next DMA)
      const int tile = cu / split, sp = cu % split;
      const int64_t m0 = (int64_t)(tile / tiles_n) * G2_BM, n0 = (int64_t)(tile % tiles_n) * BN;
      if (split == 1) {
        gemm_epilogue<C::MB, C::NB>(d, acc, (int)m0 + wm * C::MB * 16, (int)n0 + wcb, lane,
                                    ODDMAP ? (int)n0 + wodd : -1);
      } else {  // split-K: raw fp32 slab ws[sp][m][n]; gemm_splitk_reduce applies the epilogue
        float* slab = (float*)d.ws + (int64_t)sp * M * N;
#pragma unroll
        for (int a = 0; a < C::NB; ++a) {
          const int64_t n = n0 + (a == C::NB - 1 ? wodd : wcb + a * 16) + 4 * fq;
          if (n >= N) continue;
#pragma unroll
          for (int b = 0; b < C::MB; ++b) {
            const int64_t m = m0 + wm * 64 + b * 16 + fr;
            if (m < M)
              *(float4*)(slab + m * N + n) = make_float4(acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]);
          }
        }
      }
#pragma unroll
      for (int a = 0; a < C::NB; ++a)
#pragma unroll
        for (int b = 0; b < C::MB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      if ((cu += G) < units) unit_kr(cu, ckt, ckt1);
    }
    if (it + 2 < n_it) issue(stage == 0 ? 2 : stage - 1);
    stage = stage == 2 ? 0 : stage + 1;
  }
}

}  // namespace

namespace vdgemm {

template <int BN>
static int launch2(const vd_gemm_desc& d, const Plan& p, hipStream_t s) {
  const int64_t units = ((d.M + G2_BM - 1) / G2_BM) * ((d.N + BN - 1) / BN) * p.split;
  const dim3 grid((unsigned)persistent_grid(units));
  if (d.a_mode == VD_A_CONV3X3 && p.pad_end)
    hipLaunchKernelGGL((gemm2_kernel<BN, A_CONV_PAD_END>), grid, dim3(G2_NT), 0, s, d, p.a0b, p.a1b, p.wb, p.split);
  else if (d.a_mode == VD_A_CONV3X3)
    hipLaunchKernelGGL((gemm2_kernel<BN, VD_A_CONV3X3>), grid, dim3(G2_NT), 0, s, d, p.a0b, p.a1b, p.wb, p.split);
  else
    hipLaunchKernelGGL((gemm2_kernel<BN, VD_A_DENSE>), grid, dim3(G2_NT), 0, s, d, p.a0b, p.a1b, p.wb, p.split);
  const int rc = vd_launch_status();
  return rc != VD_OK || p.split == 1 ? rc : launch_splitk_reduce(d, p.split, s);
}

int launch_v2(const vd_gemm_desc& d, const Plan& p, hipStream_t s) {
  switch (p.bn) {
    case 32: return launch2<32>(d, p, s);
    case 160: return launch2<160>(d, p, s);
    default: return launch2<128>(d, p, s);
  }
}

}  // namespace vdgemm
