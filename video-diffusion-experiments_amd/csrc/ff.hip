// Fused FeedForward of the 64 x 64 level (C = 320, hidden = 1280) for gfx950 (CDNA4):
//   out = res + b2 + W2 · bf16((h + bh) · gelu_erf(g + bg)),  [h | g] = W1' · x  (+ folded LayerNorm)
// in ONE launch — the [M][1280] hidden activation is never written (vd_gemm's GEGLU launch wrote
// 335 MB at M = 131072 and the ff2 launch read it back), x is loaded once per row (the v8 GEGLU
// launch re-read it for each of its 16 column tiles) and every output row is written whole by
// one wave (v2's two 160-column tiles shared a 128-B line of each 640-B row).
//
// Orientation is gemm_common.h's: the MFMA computes C^T = W · A^T (v_mfma_f32_16x16x32_bf16, weights
// as the A operand, 16 activation rows as the B operand), so after the GEGLU epilogue lane
// (fr, fq) holds hidden values of ROW fr — a B-operand layout for a second MFMA over the hidden.
//  * A workgroup is 8 waves; each wave owns 16 whole rows per pass: x (10 k-steps = 40 VGPRs)
//    and the 16 x 320 fp32 output tile (20 blocks = 80 VGPRs) stay in registers for the pass.
//  * The hidden runs in 40 chunks of 32.  Per chunk: 4 blocks (2 sub-blocks p x {hidden, gate})
//    x 10 k-steps of W1' MFMAs, the GEGLU epilogue on the lane's 8 values, then 20 W2 MFMAs
//    (one k-step of 32 hidden per output block) — 60 MFMAs per wave between two barriers.
//  * A-row assignment: MFMA A-row r of sub-block p is W1' hidden row 32c + 8 (r >> 2) + 4p + (r & 3),
//    so lane (fr, fq)'s results of sub-blocks 0 and 1 are hidden 32c + 8 fq + 0..7 — exactly the
//    v2 kernel's B operand of k-step c, with no cross-lane move.
//  * W1' (64 rows x 320, 40 KiB) and W2 (320 x 32, 20 KiB) of a chunk reach LDS by
//    `buffer_load ... lds` into a 2-stage ring: chunk c + 1's DMA goes out right after the
//    barrier that opens chunk c, so it has a whole chunk of MFMA work to land; one raw
//    s_barrier per chunk.  The W1' image is v2's (128-B rows, 16-B chunks XOR-swizzled by
//    row & 7, rows in MFMA order); the W2 image is lane-linear (lane l of piece a holds
//    W2[16a + (l & 15)][8 (l >> 4) ..]), so each fragment read is 1 KiB contiguous.
//  * Biases and the fold's s[n] go to LDS once, in hidden order.
//  * blockIdx % 8 is the XCD; the 16-row blocks are split into 8 contiguous ranges, and every
//    workgroup of an XCD walks the weight chunks in the same order (L2 serves all but one).
// Arithmetic is the two launches', piece for piece: k-steps 0..9 ascending per hidden column
// with v8's LayerNorm fold (ones·x and x·xᵀ MFMAs, the guarded second pass), gelu_erf2 on fp32
// pairs, pack2; then one fp32 accumulator per output over hidden k-steps 0..39 ascending, hidden
// k in v2's MFMA k-slot, v2's epilogue (bias, + residual, bf16) — so the output bits equal
// vd_gemm(GEGLU) + vd_gemm(res) under the 131072-row plan (tests/test_gpu_ff_fused.py).
#include "gemm_common.h"  // lds_void, u32x4, G2_OOB (the out-of-range buffer offset)

namespace {

constexpr int FF_C = 320, FF_H = 1280, FF_NW = 8;
constexpr int FF_KS = FF_C / 32, FF_NB = FF_C / 16, FF_NCH = FF_H / 32;
constexpr int FF_W1_SUB = 64 * 128;               // a chunk's 64 W1' rows x 64 k
constexpr int FF_W1_BYTES = (FF_C / 64) * FF_W1_SUB;  // 40 KiB
constexpr int FF_W2_BYTES = FF_C * 64;            // 20 KiB
constexpr int FF_STAGE = FF_W1_BYTES + FF_W2_BYTES;
constexpr int FF_VEC = (4 * FF_H + FF_C) * 4;     // bh, bg, sh, sg (hidden order), b2
constexpr int FF_OROW = 160 * 2 + 16;             // staged half output row (bytes, padded)
static_assert(FF_NW * 16 * FF_OROW <= FF_STAGE, "output staging reuses one ring stage");
static_assert(2 * FF_STAGE + FF_VEC <= 160 * 1024, "LDS");

struct FfArgs {
  const bf16_t* x; const bf16_t* w1; const bf16_t* w2; const bf16_t* res; bf16_t* out;
  const float* b1; const float* b2; const float* s;
  int M, ldx, ld_res, ldc;
  float eps;
  uint32_t x_bytes, res_bytes, out_bytes;
};

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* lds, uint32_t voff, uint32_t soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)lds, 16, voff, soff, 0, 0);
}

template <bool LNF>
__global__ __launch_bounds__(FF_NW * 64, 1) void ff_fused_kernel(const FfArgs a) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * FF_STAGE + FF_VEC];
  float* sbh = (float*)(smem + 2 * FF_STAGE);
  float* sbg = sbh + FF_H;
  float* ssh = sbg + FF_H;
  float* ssg = ssh + FF_H;
  float* sb2 = ssg + FF_H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3, PX = gridDim.x >> 3;
  const int M = a.M;
  const int rbs = (M + 15) / 16;
  const int rb0 = (int)((int64_t)rbs * xcd / 8), rb1 = (int)((int64_t)rbs * (xcd + 1) / 8);
  // passes of this workgroup: pass t covers row blocks rb0 + (t PX + j) 8 .. + 7 (uniform over the waves)
  const int first = rb0 + j * FF_NW;
  if (first >= rb1) return;
  const int passes = (rb1 - first + PX * FF_NW - 1) / (PX * FF_NW);

  const __amdgpu_buffer_rsrc_t rw1 =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.w1, 0, (uint32_t)(2 * FF_H * FF_C * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw2 =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.w2, 0, (uint32_t)(FF_C * FF_H * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc((void*)(a.res ? a.res : a.x), 0, a.res ? a.res_bytes : 0u, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)a.out, 0, a.out_bytes, 0x00020000);

  // ---- this wave's 8 DMA pieces (1 KiB each) of a chunk: W1' piece `wid` of each of the 5
  // 64-deep sub-tiles, W2 pieces wid, 8 + wid and 16 + wid (waves 4-7: piece 8 + wid again, so
  // every wave issues the same number of loads)
  uint32_t w1off, w2off[3];
  int w2pc[3];
  {
    const int rb = lane >> 3;
    const int l = 8 * wid + rb;              // LDS row of the chunk's W1' image: block (p, hg), MFMA A-row fr
    const int b = l >> 4, p = b >> 1, hg = b & 1, r = l & 15;
    const int prow = 32 * (r >> 3) + 16 * hg + 8 * ((r >> 2) & 1) + 4 * p + (r & 3);  // packed (16-interleaved) row
    w1off = (uint32_t)(prow * (FF_C * 2) + (((lane & 7) ^ rb) * 16));
    w2pc[0] = wid; w2pc[1] = 8 + wid; w2pc[2] = wid < 4 ? 16 + wid : 8 + wid;
#pragma unroll
    for (int q = 0; q < 3; ++q) w2off[q] = (uint32_t)((16 * w2pc[q] + (lane & 15)) * (FF_H * 2) + (lane >> 4) * 16);
  }
  auto issue = [&](int c, int stage) {
    char* sb = smem + stage * FF_STAGE;
    const uint32_t so1 = (uint32_t)c * (uint32_t)(64 * FF_C * 2), so2 = (uint32_t)c * 64u;
#pragma unroll
    for (int s = 0; s < FF_C / 64; ++s) dma16(rw1, sb + s * FF_W1_SUB + wid * 1024, w1off + (uint32_t)(s * 128), so1);
#pragma unroll
    for (int q = 0; q < 3; ++q) dma16(rw2, sb + FF_W1_BYTES + w2pc[q] * 1024, w2off[q], so2);
  };
  issue(0, 0);
  for (int H = tid; H < FF_H; H += FF_NW * 64) {
    const int ph = 32 * (H >> 4) + (H & 15);
    sbh[H] = a.b1 ? a.b1[ph] : 0.f;
    sbg[H] = a.b1 ? a.b1[ph + 16] : 0.f;
    ssh[H] = LNF ? a.s[ph] : 0.f;
    ssg[H] = LNF ? a.s[ph + 16] : 0.f;
  }
  if (tid < FF_C) sb2[tid] = a.b2 ? a.b2[tid] : 0.f;

  const int fr = lane & 15, fq = lane >> 4;
  const int wcol = 16 * (fq & 1) + 8 * (fq >> 1);  // lane's column offset inside a swapped pair
  const uint32_t wl = (uint32_t)(fr * 128 + ((fq ^ (fr & 7)) << 4));  // W1' fragment (block 0, even k-step)
  bf16x8 x[FF_KS];
  auto load_x = [&](int rb) {
    const int m = rb * 16 + fr;
    const uint32_t o = (rb < rb1 && m < M) ? (uint32_t)m * (uint32_t)(a.ldx * 2) + (uint32_t)(fq * 16) : G2_OOB;
#pragma unroll
    for (int ks = 0; ks < FF_KS; ++ks)
      x[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rx, o + (uint32_t)(ks * 64), 0, 0));
  };
  int r = first + wid;
  load_x(r);
  char* obuf = smem + FF_STAGE + wid * 16 * FF_OROW;  // stage 1, after the pass's last chunk

  for (int t = 0; t < passes; ++t) {
    // ---- LayerNorm statistics of the wave's 16 rows (v8's: ones·x and x·xᵀ per k-step)
    float nmean = 0.f, rstd = 1.f;
    if constexpr (LNF) {
      f32x4 sacc = f32x4{0.f, 0.f, 0.f, 0.f}, gacc = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16x8 ones = __builtin_bit_cast(bf16x8, make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u));
#pragma unroll
      for (int ks = 0; ks < FF_KS; ++ks) {
        sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, x[ks], sacc, 0, 0, 0);
        gacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[ks], x[ks], gacc, 0, 0, 0);
      }
      const int j3 = fr & 3;
      const float gd = j3 == 0 ? gacc[0] : j3 == 1 ? gacc[1] : j3 == 2 ? gacc[2] : gacc[3];
      const float sxx = __shfl(gd, fr + 16 * (fr >> 2), 64);
      constexpr float RK = 1.0f / (float)FF_C;
      const float mean = sacc[0] * RK;
      const float var = fmaf(sxx, RK, -mean * mean);
      rstd = rsqrtf(row_var_guarded<FF_KS>(x, mean, var, RK) + a.eps);
      nmean = -mean;
    }
    // the pass's x rows are waited for HERE: left to the first MFMA of the chunk loop, hipcc
    // waits vmcnt(0) there in every chunk and drains the weight DMA it should leave in flight
#pragma unroll
    for (int ks = 0; ks < FF_KS; ++ks) asm volatile("" : "+v"(x[ks]));
    f32x4 acc[FF_NB];
#pragma unroll
    for (int n = 0; n < FF_NB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int c = 0; c < FF_NCH; ++c) {
      const int stage = c & 1;
      // chunk c's DMA (issued one chunk ago) has landed; every wave is done reading stage ^ 1
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // the chunk's bias / s[n] values leave LDS before the next DMA goes out: hipcc waits
      // vmcnt(0) ahead of any typed LDS read it sees behind a pending LDS-DMA, which would
      // drain the prefetch in the middle of the chunk
      float4 tbh[2], tbg[2], tsh[2], tsg[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int H0 = 32 * c + 8 * fq + 4 * p;
        tbh[p] = *(const float4*)(sbh + H0);
        tbg[p] = *(const float4*)(sbg + H0);
        if constexpr (LNF) {
          tsh[p] = *(const float4*)(ssh + H0);
          tsg[p] = *(const float4*)(ssg + H0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (c + 1 < FF_NCH) issue(c + 1, stage ^ 1);
      else if (t + 1 < passes) issue(0, 0);
      const char* sb = smem + stage * FF_STAGE;
      // ---- GEGLU half: blocks b = 2p + hg, 10 ascending k-steps, fragments two k-steps ahead
      f32x4 hg[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) hg[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      bf16x8 wf[3][4];
      auto read_w1 = [&](bf16x8 (&f)[4], int ks) {
        const char* p = sb + (ks >> 1) * FF_W1_SUB + ((ks & 1) ? (wl ^ 64u) : wl);
#pragma unroll
        for (int b = 0; b < 4; ++b) f[b] = *(const bf16x8*)(p + b * 2048);
      };
      read_w1(wf[0], 0);
      read_w1(wf[1], 1);
#pragma unroll
      for (int ks = 0; ks < FF_KS; ++ks) {
        if (ks + 2 < FF_KS) read_w1(wf[(ks + 2) % 3], ks + 2);
#pragma unroll
        for (int b = 0; b < 4; ++b) hg[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks % 3][b], x[ks], hg[b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // the first half of the chunk's W2 fragments goes out ahead of the epilogue's VALU
      const char* s2 = sb + FF_W1_BYTES + lane * 16;
      constexpr int NA = 6, NBB = FF_NB - NA;  // W2 fragments read ahead of / behind the epilogue
      bf16x8 w2a[NA], w2b[NBB];
#pragma unroll
      for (int n = 0; n < NA; ++n) w2a[n] = *(const bf16x8*)(s2 + n * 1024);
      // the pass's last GEGLU half is done with x: the next pass's rows load under the rest
      if (c == FF_NCH - 1 && t + 1 < passes) load_x(r + PX * FF_NW);
      // ---- GEGLU epilogue (v8's arithmetic): the lane's hidden 32c + 8 fq + 4p + 0..3
      uint32_t hb[4];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const float4 th = tbh[p], tg = tbg[p];
        const float thv[4] = {th.x, th.y, th.z, th.w}, tgv[4] = {tg.x, tg.y, tg.z, tg.w};
        float hv[4], gv[4];
        if constexpr (LNF) {
          const float4 sh = tsh[p], sg = tsg[p];
          const float shv[4] = {sh.x, sh.y, sh.z, sh.w}, sgv[4] = {sg.x, sg.y, sg.z, sg.w};
#pragma unroll
          for (int j4 = 0; j4 < 4; ++j4) {
            hv[j4] = fmaf(rstd, fmaf(nmean, shv[j4], hg[2 * p][j4]), thv[j4]);
            gv[j4] = fmaf(rstd, fmaf(nmean, sgv[j4], hg[2 * p + 1][j4]), tgv[j4]);
          }
        } else {
#pragma unroll
          for (int j4 = 0; j4 < 4; ++j4) {
            hv[j4] = hg[2 * p][j4] + thv[j4];
            gv[j4] = hg[2 * p + 1][j4] + tgv[j4];
          }
        }
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          const f32x2 go = gelu_erf2(f32x2{gv[2 * h2], gv[2 * h2 + 1]});
          const f32x2 oo = f32x2{hv[2 * h2], hv[2 * h2 + 1]} * go;
          hb[2 * p + h2] = pack2(oo[0], oo[1]);
        }
      }
      const bf16x8 hf = __builtin_bit_cast(bf16x8, make_uint4(hb[0], hb[1], hb[2], hb[3]));
      __builtin_amdgcn_sched_barrier(0);
      // ---- ff2 half: hidden k-step c of every output block
#pragma unroll
      for (int n = 0; n < NBB; ++n) w2b[n] = *(const bf16x8*)(s2 + (NA + n) * 1024);
#pragma unroll
      for (int n = 0; n < NA; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2a[n], hf, acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NBB; ++n) acc[NA + n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2b[n], hf, acc[NA + n], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- epilogue (v2's arithmetic): residual rows, bias from LDS, whole 640-B rows through LDS
    u32x4 rsv[FF_NB / 2];
    {
      const int m = r * 16 + fr;
#pragma unroll
      for (int pr = 0; pr < FF_NB / 2; ++pr) {
        const uint32_t off = (r < rb1 && m < M) ? (uint32_t)(m * a.ld_res + pr * 32 + wcol) * 2u : G2_OOB;
        rsv[pr] = __builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave is done reading stage 1 (the last chunk's)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int n = half * (FF_NB / 2); n < (half + 1) * (FF_NB / 2); n += 2) {
        const int cc = n * 16 + wcol;
        const float4 t0 = *(const float4*)(sb2 + cc), t1 = *(const float4*)(sb2 + cc + 4);
        const float bv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        float o[8];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          auto rp = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[n][jj]), __float_as_uint(acc[n + 1][jj]),
                                                     false, false);
          o[jj] = __uint_as_float(rp[0]) + bv[jj];
          o[4 + jj] = __uint_as_float(rp[1]) + bv[4 + jj];
        }
        if (a.res) {
          float rf[8];
          const u32x4 rv = rsv[n / 2];
          unpack8(make_uint4(rv[0], rv[1], rv[2], rv[3]), rf);
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) o[jj] += rf[jj];
        }
        *(uint4*)(obuf + fr * FF_OROW + (cc - half * 160) * 2) = pack8(o);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int it = 0; it < 5; ++it) {  // 16 rows x 320 B (in-order LDS: no barrier within the wave)
        const int q = it * 64 + lane, row = q / 20, ch = q - row * 20;
        const uint4 v = *(const uint4*)(obuf + row * FF_OROW + ch * 16);
        const int m = r * 16 + row;
        const uint32_t off = (r < rb1 && m < M) ? (uint32_t)(m * a.ldc + half * 160 + ch * 8) * 2u : G2_OOB;
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{v.x, v.y, v.z, v.w}, ro, off, 0, 0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    r += PX * FF_NW;
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the device's CU count, read once per process (as gemm.hip's num_cus; its own, so that this file
// needs no symbol of the GEMM objects and links beside any of them, tools/gemm_ab.py)
int ff_num_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      return n;
    return 256;
  }();
  return cus;
}

}  // namespace

// The plan's shape rule: C = 320, hidden = 4C, M >= 65536.  Measured (tools/gemm_ab.py
// GEMM_AB_CASES=ff, profiles/ff_fused_l1_ab.txt): at M = 131072 (4 passes of the grid) the
// fused launch beats vd_gemm(GEGLU) + vd_gemm(res), 399 vs 457 us folded; at a frame-sharded
// rank's M = 16384 and 8192 (half a pass and less: the 40-chunk weight walk is not amortised)
// it loses, 86 vs 69 us and 78 vs 43 us, so those keep the two launches.
extern "C" int vd_ff_fused_takes(int64_t M, int64_t C, int64_t hidden) {
  return C == FF_C && hidden == FF_H && M >= 65536 && M * FF_C * 2 < (int64_t)G2_OOB;
}

extern "C" int vd_ff_fused(const void* x, int64_t ldx, int64_t M, int64_t C, int64_t hidden, const void* w1,
                           const float* b1, const float* ln_fold_s, float ln_eps, const void* w2, const float* b2,
                           const void* res, int64_t ld_res, void* out, int64_t ldc, vd_stream_t stream) {
  VD_CHECK_ARG(M >= 0 && C > 0 && hidden > 0);
  if (C != FF_C || hidden != FF_H) return VD_EUNSUPPORTED;
  if (M == 0) return VD_OK;
  VD_CHECK_ARG(x && w1 && w2 && out && al16(x) && al16(w1) && al16(w2) && al16(out));
  VD_CHECK_ARG(ldx >= FF_C && ldx % 8 == 0 && ldc >= FF_C && ldc % 8 == 0);
  VD_CHECK_ARG(!res || (al16(res) && ld_res >= FF_C && ld_res % 8 == 0));
  VD_CHECK_ARG(!b1 || al16(b1));
  VD_CHECK_ARG(!b2 || al16(b2));
  VD_CHECK_ARG(!ln_fold_s || (al16(ln_fold_s) && ln_eps >= 0.f));
  VD_CHECK_ARG(M * ldx * 2 < (int64_t)G2_OOB && M * ldc * 2 < (int64_t)G2_OOB &&
               (!res || M * ld_res * 2 < (int64_t)G2_OOB));
  FfArgs a;
  a.x = (const bf16_t*)x; a.w1 = (const bf16_t*)w1; a.w2 = (const bf16_t*)w2; a.res = (const bf16_t*)res;
  a.out = (bf16_t*)out; a.b1 = b1; a.b2 = b2; a.s = ln_fold_s;
  a.M = (int)M; a.ldx = (int)ldx; a.ld_res = (int)ld_res; a.ldc = (int)ldc;
  a.eps = ln_eps;
  // the last row ends at its C-th column, not at its stride
  a.x_bytes = (uint32_t)(((M - 1) * ldx + FF_C) * 2);
  a.res_bytes = res ? (uint32_t)(((M - 1) * ld_res + FF_C) * 2) : 0u;
  a.out_bytes = (uint32_t)(((M - 1) * ldc + FF_C) * 2);
  const int cus = ff_num_cus();
  const int per_xcd = cus >= 8 ? cus / 8 : 1;  // one workgroup per CU, blockIdx % 8 = XCD
  const dim3 grid((unsigned)(8 * per_xcd)), block(FF_NW * 64);
  hipStream_t s = (hipStream_t)stream;
  if (ln_fold_s) hipLaunchKernelGGL((ff_fused_kernel<true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((ff_fused_kernel<false>), grid, block, 0, s, a);
  return vd_launch_status();
}
