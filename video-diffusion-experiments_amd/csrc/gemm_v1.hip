// ============================================================================ v1
// The register-staged GEMM / implicit-GEMM conv that takes every valid descriptor (small and
// ragged shapes in the plan), and v9, its skinny form for M <= 16.
// Tile BM x BN x 64, 256 threads = 4 waves as 2(M) x 2(N); operands staged
// global -> registers -> LDS (register staging so the conv gather, the channel
// concat and the nearest-x2 upsample happen in the load), double-buffered LDS
// with the next tile's global loads issued before the MFMAs of the current one
// (cdna_hip_programming.md T14), 16-B chunks XOR-swizzled by (row & 7) so the
// ds_read_b128 fragment reads spread over the bank row (T2), and an XCD-aware
// tile order (T1).
#include "gemm_common.h"

namespace {

template <int BM, int BN, int MODE>
__global__ __launch_bounds__(NT, 2) void gemm_kernel(const vd_gemm_desc d) {
  constexpr int RA = BM / 32;        // A chunks staged per thread
  constexpr int RW = BN / 32;        // W chunks staged per thread
  constexpr int MB = BM / 2 / 16;    // 16-row m blocks per wave
  constexpr int NB = BN / 2 / 16;    // 16-row n blocks per wave
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * (BM + BN) * BK];
  bf16_t* As = smem;
  bf16_t* Ws = smem + 2 * BM * BK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  const int64_t M = d.M, N = d.N, K = d.K;
  const int tiles_n = (int)((N + BN - 1) / BN);
  const int tiles_m = (int)((M + BM - 1) / BM);
  const int id = xcd_remap(blockIdx.x, tiles_n * tiles_m);
  const int64_t m0 = (int64_t)(id / tiles_n) * BM;
  const int64_t n0 = (int64_t)(id % tiles_n) * BN;

  const int sc = tid & 7;    // staged chunk (8 bf16) within the 64-wide K tile
  const int sr = tid >> 3;   // staged row base (rows sr + 32*i)

  const bf16_t* a0 = (const bf16_t*)d.a0;
  const bf16_t* a1 = (const bf16_t*)d.a1;
  const bf16_t* w = (const bf16_t*)d.w;

  // Per staged A row: pixel coordinates for the conv gather.  pimg = the input image of
  // temporal tap 0, pfr = its frame index inside the video (valid range [0, frames_in)).
  int pimg[RA], pfr[RA], poh[RA], pow_[RA];
  bool prow[RA];
  int cin = 0, hgrid = 0, wgrid = 0;
  if constexpr (mode_is_conv(MODE)) {
    cin = (int)d.K / (d.ks * d.ks * d.kt);
    hgrid = d.upsample ? 2 * d.h_in : d.h_in;
    wgrid = d.upsample ? 2 * d.w_in : d.w_in;
    const int hw = d.h_out * d.w_out;
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      const int64_t m = m0 + sr + 32 * i;
      prow[i] = m < M;
      const int mm = prow[i] ? (int)m : 0;
      const int img = mm / hw;
      const int vid = img / d.frames_out;
      pfr[i] = img - vid * d.frames_out + d.t_off - d.kt / 2;
      pimg[i] = vid * d.frames_in + pfr[i];
      const int p = mm - img * hw;
      poh[i] = p / d.w_out;
      pow_[i] = p - poh[i] * d.w_out;
    }
  }

  uint4 ra[RA], rw[RW];

  auto load_tile = [&](int kt) {
    const int64_t k = (int64_t)kt * BK + sc * 8;
    if constexpr (MODE == VD_A_DENSE) {
      const bool in0 = k < d.k0;
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        const int64_t m = m0 + sr + 32 * i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (m < M && k < K) {
          const bf16_t* p = in0 ? a0 + m * d.lda0 + k : a1 + m * d.lda1 + (k - d.k0);
          v = *(const uint4*)p;
        }
        ra[i] = v;
      }
    } else {
      const bool kin = k < K;
      const int tap27 = kin ? (int)(k / cin) : 0;
      const int ci = (int)k - tap27 * cin;
      const int ks2 = d.ks * d.ks;
      const int dt = tap27 / ks2, tap = tap27 - ks2 * dt;
      const int dy = d.ks == 3 ? tap / 3 : 1, dx = d.ks == 3 ? tap - 3 * (tap / 3) : 1;
      const bool in0 = ci < d.k0;
      const bf16_t* base = in0 ? a0 + ci : a1 + (ci - d.k0);
      const int64_t ld = in0 ? d.lda0 : d.lda1;
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        int ih = poh[i] * d.stride + dy - conv_pad_lo<MODE>;
        int iw = pow_[i] * d.stride + dx - conv_pad_lo<MODE>;
        const int fin = pfr[i] + dt;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (kin && prow[i] && ih >= 0 && ih < hgrid && iw >= 0 && iw < wgrid && fin >= 0 && fin < d.frames_in) {
          ih >>= d.upsample;
          iw >>= d.upsample;
          const int64_t pix = ((int64_t)(pimg[i] + dt) * d.h_in + ih) * d.w_in + iw;
          v = *(const uint4*)(base + pix * ld);
        }
        ra[i] = v;
      }
    }
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int64_t n = n0 + sr + 32 * i;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (n < N && k < K) v = *(const uint4*)(w + n * d.ldw + k);
      rw[i] = v;
    }
  };
  auto store_tile = [&](int buf) {
    bf16_t* as = As + buf * BM * BK;
    bf16_t* ws = Ws + buf * BN * BK;
#pragma unroll
    for (int i = 0; i < RA; ++i) *(uint4*)(as + lds_off(sr + 32 * i, sc)) = ra[i];
#pragma unroll
    for (int i = 0; i < RW; ++i) *(uint4*)(ws + lds_off(sr + 32 * i, sc)) = rw[i];
  };

  f32x4 acc[NB][MB];
#pragma unroll
  for (int a = 0; a < NB; ++a)
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (int)((K + BK - 1) / BK);
  load_tile(0);
  store_tile(0);
  __syncthreads();

  const int fr = lane & 15;   // fragment row within a 16-block
  const int fq = lane >> 4;   // which 8-wide k slice (0..3)
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    const bf16_t* as = As + cur * BM * BK;
    const bf16_t* ws = Ws + cur * BN * BK;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8 wf[NB], xf[MB];
#pragma unroll
      for (int a = 0; a < NB; ++a)
        wf[a] = *(const bf16x8*)(ws + lds_off(wn * (BN / 2) + a * 16 + fr, ks * 4 + fq));
#pragma unroll
      for (int b = 0; b < MB; ++b)
        xf[b] = *(const bf16x8*)(as + lds_off(wm * (BM / 2) + b * 16 + fr, ks * 4 + fq));
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < MB; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a], xf[b], acc[a][b], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tile(cur ^ 1);
    __syncthreads();
  }

  if (d.rmap_inner)
    gemm_epilogue<MB, NB, true>(d, acc, (int)m0 + wm * MB * 16, (int)n0 + wn * (BN / 2), lane);
  else
    gemm_epilogue<MB, NB>(d, acc, (int)m0 + wm * MB * 16, (int)n0 + wn * (BN / 2), lane);
}

// ============================================================================ v9
// Skinny GEMM, M <= 16: the time-embedding MLP and the resnets' concatenated time_emb_proj (M = the
// UNet batch, 2 with CFG) — weight streaming, HBM-bound.  v1's 128 x 160 tiles put these on 8 / 126
// workgroups (22 / 31 us per launch at N = 1280 / 20160).  One wave owns 16 output columns and all
// of K; its MFMA chain is v1's (C^T = W . A^T by v_mfma_f32_16x16x32_bf16, k ascending, one
// accumulator, zero-filled past K), so the result is bit-identical to v1's.  The fragments come
// straight from global memory (no LDS): lane (fr, fq) holds W row n0 + fr and A row fr (zero for
// fr >= M), k slice 8*fq .. +7 of each 32-k step; G9_U steps of loads are in flight ahead of the
// MFMAs that consume the previous G9_U.  The epilogue is gemm_epilogue's narrow path (MB = NB = 1).
__global__ __launch_bounds__(G9_NW * 64) void gemm9_kernel(const vd_gemm_desc d) {
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = (blockIdx.x * G9_NW + (threadIdx.x >> 6)) * 16;
  const int N = (int)d.N, M = (int)d.M, K = (int)d.K;
  if (n0 >= N) return;  // wave-uniform; no barriers below
  const bool nok = n0 + fr < N, mok = fr < M;
  const bf16_t* wp = (const bf16_t*)d.w + (int64_t)(nok ? n0 + fr : 0) * d.ldw + 8 * fq;
  const bf16_t* ap = (const bf16_t*)d.a0 + (int64_t)(mok ? fr : 0) * d.lda0 + 8 * fq;
  const int nsteps = (K + 31) / 32;
  uint4 wc[G9_U], ac[G9_U], wn[G9_U], an[G9_U];
  auto load = [&](int s0, uint4 (&wv)[G9_U], uint4 (&av)[G9_U]) {
#pragma unroll
    for (int u = 0; u < G9_U; ++u) {
      const int k = (s0 + u) * 32;
      const bool kok = k + 8 * fq < K;
      wv[u] = nok && kok ? *(const uint4*)(wp + k) : make_uint4(0, 0, 0, 0);
      av[u] = mok && kok ? *(const uint4*)(ap + k) : make_uint4(0, 0, 0, 0);
    }
  };
  f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
  load(0, wc, ac);
  for (int s0 = 0; s0 < nsteps; s0 += G9_U) {
    if (s0 + G9_U < nsteps) load(s0 + G9_U, wn, an);
#pragma unroll
    for (int u = 0; u < G9_U; ++u)
      if (s0 + u < nsteps)
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wc[u]),
                                                             __builtin_bit_cast(bf16x8, ac[u]), acc[0][0], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < G9_U; ++u) {
      wc[u] = wn[u];
      ac[u] = an[u];
    }
  }
  gemm_epilogue<1, 1>(d, acc, 0, n0, lane);
}

}  // namespace

namespace vdgemm {

template <int BM, int BN>
static int launch(const vd_gemm_desc& d, const Plan& p, hipStream_t s) {
  const int64_t tiles = ((d.M + BM - 1) / BM) * ((d.N + BN - 1) / BN);
  if (tiles > 0x7fffffff) return VD_EINVAL;
  if (d.a_mode == VD_A_CONV3X3 && p.pad_end)
    hipLaunchKernelGGL((gemm_kernel<BM, BN, A_CONV_PAD_END>), dim3((unsigned)tiles), dim3(NT), 0, s, d);
  else if (d.a_mode == VD_A_CONV3X3)
    hipLaunchKernelGGL((gemm_kernel<BM, BN, VD_A_CONV3X3>), dim3((unsigned)tiles), dim3(NT), 0, s, d);
  else
    hipLaunchKernelGGL((gemm_kernel<BM, BN, VD_A_DENSE>), dim3((unsigned)tiles), dim3(NT), 0, s, d);
  return vd_launch_status();
}

int launch_v1(const vd_gemm_desc& d, const Plan& p, hipStream_t s) {
  switch (p.bn) {
    case 128: return launch<128, 128>(d, p, s);
    case 64: return launch<128, 64>(d, p, s);
    case 160: return launch<128, 160>(d, p, s);
    default: return VD_EINVAL;
  }
}

int launch_v9(const vd_gemm_desc& d, hipStream_t s) {
  const int64_t waves = (d.N + 15) / 16;
  hipLaunchKernelGGL(gemm9_kernel, dim3((unsigned)((waves + G9_NW - 1) / G9_NW)), dim3(G9_NW * 64), 0, s, d);
  return vd_launch_status();
}

}  // namespace vdgemm
