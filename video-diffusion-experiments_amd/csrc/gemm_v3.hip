// ============================================================================ v3
// 256x256 tile, 8 waves as 2(M) x 4(N) (128 x 64 per wave: 0.375 LDS fragment
// reads per MFMA vs 0.45 for v2's 64 x 80), after the 8-phase template of
// cdna_hip_programming.md §5 "The 256² 8-phase template":
//  * a K-tile (BK = 64) is 4 phases, each one quadrant of the wave's C
//    (64 m x 32 n x K 64 = 16 MFMAs): Q(x0,w0) Q(x0,w1) Q(x1,w1) Q(x1,w0), so
//    the phases read 12 / 4 / 8 / 0 fragments (W0+X0, W1, X1, -);
//  * each K-tile's operands are four 16-KiB parts — X0 = A rows with
//    (r & 127) < 64, X1 the other A rows, W0 = W rows with (n & 63) < 32, W1 the
//    rest — one part DMA'd (buffer_load ... lds, 2 instructions per wave) per
//    phase, 6-7 phases before its first read, into the stage of the K-tile two
//    back (2 x 64 KiB); every part is restaged >= 1 phase after its last read
//    (lgkmcnt(0) retired the reads before the phase's MFMAs) and waited for by
//    a uniform counted vmcnt(10) (5 parts in flight) before the barrier ahead of
//    its first read;
//  * phase = [ds_reads | DMA | vmcnt] barrier lgkmcnt(0) setprio(1) MFMAs
//    setprio(0) barrier, and the wr = 1 wave group runs ONE BARRIER BEHIND the
//    wr = 0 group: on every SIMD (one wave of each group) one wave issues MFMAs
//    while the other reads LDS and issues DMA (ping-pong);
//  * the A (X) parts a wave group reads are DMA'd by that group only, so the
//    stagger never lets one group overwrite rows the other has yet to read; the
//    W parts, read by both groups, are restaged >= 2 phases after their reads.
// Persistent (round 2): a workgroup walks units lid, lid + G, ... (unit = output tile or
// one split-K slice of it, XCD-aware order with the N tiles of an A row-panel adjacent),
// and the K-tiles of all its units form ONE flat stream: the DMA of the next unit's first
// two K-tiles goes out during the last K-tiles of the current one, so the prologue's HBM
// burst and most of the epilogue's store tail overlap MFMA work (per-tile fixed cost,
// profiles/r02_v3_k_sweep.txt: 9.4 us per 256^2 tile vs 4.8 for hipBLASLt).  At a unit
// boundary the two wave groups re-align (group 0 one extra barrier), both run the
// epilogue, and group 1 re-staggers (one extra barrier) before the next unit's phase 0.
// Grid = units gives one unit per workgroup (the round-1 non-persistent kernel).
#include "gemm_common.h"

namespace {

constexpr int G3_A_BYTES = G3_BM * BK * 2;     // 32 KiB
constexpr int G3_STAGE = 2 * G3_A_BYTES;       // A + W: 64 KiB
// Load-free epilogue (round 2): for plain bf16 outputs (no residual / row bias, unsplit) with
// N <= G3_BIAS_N the whole bias vector is copied into LDS once, before the first DMA, and the
// epilogue is v5's epi_fast (bias from LDS, unconditional buffer stores).  gemm_epilogue's
// global bias loads made hipcc wait vmcnt(0) at every unit boundary — draining the next
// unit's two K-tiles of DMA under the epilogue (20 units per CU at the L1 GEGLU).
constexpr int G3_BIAS_N = 5120;

struct G3Cursor {  // a position (unit, local K-tile) in the workgroup's flat K-tile stream
  int u, t, kt0, nk, m0, n0;
};

template <int MODE>
__global__ __launch_bounds__(G3_NT, 1) void gemm3_kernel(const vd_gemm_desc d, uint32_t a0_bytes,
                                                         uint32_t a1_bytes, uint32_t w_bytes, int split,
                                                         int fast) {
  static_assert(MODE == VD_A_DENSE, "gemm3: dense A only");
  __shared__ __attribute__((aligned(1024))) char smem[2 * G3_STAGE + G3_BIAS_N * 4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;
  const int M = (int)d.M, N = (int)d.N;
  const int tiles_n = (N + G3_BN - 1) / G3_BN;
  const int units = ((M + G3_BM - 1) / G3_BM) * tiles_n * split;
  const int lid = xcd_remap(blockIdx.x, gridDim.x), G = gridDim.x;
  const int nk_all = (int)(d.K / BK);

  auto set_unit = [&](G3Cursor& c, int u) {
    c.u = u;
    c.t = 0;
    if (u < units) {
      const int tile = u / split, sp = u % split;
      c.kt0 = split == 1 ? 0 : nk_all * sp / split;  // 32-bit: nk_all * split < 2^31
      c.nk = (split == 1 ? nk_all : nk_all * (sp + 1) / split) - c.kt0;
      c.m0 = (tile / tiles_n) * G3_BM;
      c.n0 = (tile % tiles_n) * G3_BN;
    }
  };
  auto advance = [&](G3Cursor& c) {
    if (++c.t == c.nk) set_unit(c, c.u + G);
  };
  int total = 0;  // K-tiles this workgroup streams
  for (int u = lid; u < units; u += G) {
    G3Cursor c;
    set_unit(c, u);
    total += c.nk;
  }
  if (total == 0) return;

  const int rb = lane >> 3;
  const uint32_t lc16 = (uint32_t)(((lane & 7) ^ rb) * 16);
  const __amdgpu_buffer_rsrc_t ra0 = __builtin_amdgcn_make_buffer_rsrc((void*)d.a0, 0, a0_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ra1 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(d.a1 ? d.a1 : d.a0), 0, d.a1 ? a1_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)d.w, 0, w_bytes, 0x00020000);
  const uint32_t lda0b = (uint32_t)d.lda0 * 2, lda1b = (uint32_t)d.lda1 * 2, ldwb = (uint32_t)d.ldw * 2;
  float* const bias_lds = (float*)(smem + 2 * G3_STAGE);
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(d.out, 0, (uint32_t)(M * d.ldc * 2), 0x00020000);
  if (fast) {  // the bias (or zeros) into LDS before any DMA is in flight; the prologue's
               // lgkmcnt(0) + s_barrier publish it
    for (int i = 4 * tid; i < N; i += 4 * G3_NT)
      *(float4*)(bias_lds + i) = d.bias ? *(const float4*)(d.bias + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    __builtin_amdgcn_sched_barrier(0);
  }

  // DMA slots (wave-uniform LDS offsets; per-lane source rows from the cursor's tile): X part
  // q, slot j covers A rows 128*wr + 64*q + 8*(2*wc + j) + 0..7; W part q, slot j covers W
  // rows 64*c + 32*q + rr + 0..7 with (c, rr) from g = 2*wid + j.
  auto dma_x = [&](int q, const G3Cursor& c, int T) {  // X part q of flat K-tile T (at cursor c)
    char* st = smem + (T & 1) * G3_STAGE;
    const int kb = (c.kt0 + c.t) * BK;
    const bool s0 = kb < (int)d.k0;
    const uint32_t koff = (uint32_t)(s0 ? kb : kb - (int)d.k0) * 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int xr = 128 * wr + 64 * q + 8 * (2 * wc + j);
      int m = c.m0 + xr + rb;
      m = m < M ? m : M - 1;
      dma16(s0 ? ra0 : ra1, st + xr * 128, (uint32_t)m * (s0 ? lda0b : lda1b) + lc16 + koff);
    }
  };
  auto dma_w = [&](int q, const G3Cursor& c, int T) {
    char* st = smem + (T & 1) * G3_STAGE;
    const uint32_t koff = (uint32_t)((c.kt0 + c.t) * BK) * 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int g = 2 * wid + j;
      const int wrow = 64 * (g >> 2) + 32 * q + 8 * (g & 3);
      int n = c.n0 + wrow + rb;
      n = n < N ? n : N - 1;
      dma16(rw, st + G3_A_BYTES + wrow * 128, (uint32_t)n * ldwb + lc16 + koff);
    }
  };

  // fragment LDS offsets (bytes within a stage): rows differ by multiples of 16
  // between the blocks of one operand, so the (row & 7) XOR is shared
  const int fr = lane & 15, fq = lane >> 4;
  uint32_t xl[2][2], wl[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      xl[h][ks] = 2 * lds_off(128 * wr + 64 * h + fr, ks * 4 + fq);
      wl[h][ks] = G3_A_BYTES + 2 * lds_off(64 * wc + 32 * h + fr, ks * 4 + fq);
    }

  f32x4 acc[4][8];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // cursors of flat K-tiles T (compute), T+1 and T+2 (DMA)
  G3Cursor c0, c1, c2;
  set_unit(c0, lid);
  c1 = c0;
  advance(c1);
  c2 = c1;
  advance(c2);
  // ---- prologue: K-tile 0 complete, K-tile 1's X0/W0/W1 in flight
  dma_x(0, c0, 0); dma_w(0, c0, 0); dma_w(1, c0, 0); dma_x(1, c0, 0);
  if (total > 1) {
    dma_x(0, c1, 1); dma_w(0, c1, 1); dma_w(1, c1, 1);
    wait_vm<10>();
  } else {
    wait_vm<0>();
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wr == 1) __builtin_amdgcn_s_barrier();  // the stagger

  bf16x8 w0f[2][2], w1f[2][2], xf[4][2];
  for (int T = 0; T < total; ++T) {
    const char* st = smem + (T & 1) * G3_STAGE;
    const bool deep = T + 2 < total;
#define G3_SYNC_MFMA(H, G_, WF)                                                                    \
    if (deep) wait_vm<10>(); else wait_vm<0>();                                                     \
    __builtin_amdgcn_s_barrier();                                                                   \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                              \
    __builtin_amdgcn_s_setprio(1);                                                                  \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                \
      _Pragma("unroll") for (int a = 0; a < 2; ++a)                                                 \
        _Pragma("unroll") for (int b = 0; b < 4; ++b)                                               \
          acc[2 * (G_) + a][4 * (H) + b] =                                                          \
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(WF[a][ks], xf[b][ks], acc[2 * (G_) + a][4 * (H) + b], 0, 0, 0); \
    __builtin_amdgcn_s_setprio(0);                                                                  \
    __builtin_amdgcn_s_barrier();
    // ---- phase 0: read W0, X0; DMA X1 of T+1; Q(x0, w0)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) w0f[a][ks] = *(const bf16x8*)(st + wl[0][ks] + a * 16 * BK * 2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) xf[b][ks] = *(const bf16x8*)(st + xl[0][ks] + b * 16 * BK * 2);
    if (T + 1 < total) dma_x(1, c1, T + 1);
    G3_SYNC_MFMA(0, 0, w0f)
    // ---- phase 1: read W1; DMA X0 of T+2; Q(x0, w1)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) w1f[a][ks] = *(const bf16x8*)(st + wl[1][ks] + a * 16 * BK * 2);
    if (deep) dma_x(0, c2, T + 2);
    G3_SYNC_MFMA(0, 1, w1f)
    // ---- phase 2: read X1; DMA W0 of T+2; Q(x1, w1)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) xf[b][ks] = *(const bf16x8*)(st + xl[1][ks] + b * 16 * BK * 2);
    if (deep) dma_w(0, c2, T + 2);
    G3_SYNC_MFMA(1, 1, w1f)
    // ---- phase 3: DMA W1 of T+2; Q(x1, w0)
    if (deep) dma_w(1, c2, T + 2);
    G3_SYNC_MFMA(1, 0, w0f)
#undef G3_SYNC_MFMA
    if (c0.t + 1 == c0.nk) {  // unit finished
      if (wr == 0) __builtin_amdgcn_s_barrier();  // re-align the groups
      const int mbase = c0.m0 + 128 * wr, nbase = c0.n0 + 64 * wc;
      if (fast) {
        epi_fast<8, 4>(d, acc, mbase, nbase, lane, bias_lds + c0.n0, c0.n0, rout);
      } else if (split == 1) {
        gemm_epilogue<8, 4>(d, acc, mbase, nbase, lane);
      } else {  // split-K: raw fp32 slab ws[sp][m][n]; gemm_splitk_reduce applies the epilogue
        float* slab = (float*)d.ws + (int64_t)(c0.u % split) * d.M * d.N;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int64_t n = nbase + a * 16 + 4 * fq;
          if (n >= N) continue;
#pragma unroll
          for (int b = 0; b < 8; ++b) {
            const int64_t m = mbase + b * 16 + fr;
            if (m < M) *(float4*)(slab + m * d.N + n) = make_float4(acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]);
          }
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (wr == 1 && T + 1 < total) __builtin_amdgcn_s_barrier();  // re-stagger
    }
    advance(c0);
    advance(c1);
    advance(c2);
  }
}

}  // namespace

namespace vdgemm {

int launch_v3(const vd_gemm_desc& d, const Plan& p, hipStream_t s) {
  const int64_t units = ((d.M + G3_BM - 1) / G3_BM) * ((d.N + G3_BN - 1) / G3_BN) * p.split;
  if (units > 0x7fffffff) return VD_EINVAL;
  const int fast = p.split == 1 && !d.res && !d.rowbias && !d.out_f32 && !d.rmap_inner && d.N % 8 == 0 &&
                   d.N <= G3_BIAS_N && d.ldc % 8 == 0 && ((uintptr_t)d.out & 15) == 0 &&
                   d.M * d.ldc * 2 < (int64_t)G2_OOB;
  hipLaunchKernelGGL((gemm3_kernel<VD_A_DENSE>), dim3((unsigned)persistent_grid(units)), dim3(G3_NT), 0, s, d, p.a0b,
                     p.a1b, p.wb, p.split, fast);
  const int rc = vd_launch_status();
  return rc != VD_OK || p.split == 1 ? rc : launch_splitk_reduce(d, p.split, s);
}

}  // namespace vdgemm
