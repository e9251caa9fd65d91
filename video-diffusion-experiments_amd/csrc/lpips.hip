// LPIPS (AlexNet, lpips.LPIPS(net='alex', version='0.1'), eval mode) over consecutive frames:
// the perceptual half of experiments/06_measure_grid_search.py (LPIPSMetric, :122-154), in exact
// fp32 on the f32-input MFMA (v_mfma_f32_16x16x4_f32: bit-for-bit a k-ordered fmaf chain).
//
//   vd_conv2d_f32   NHWC fp32 implicit-GEMM convolution, any kernel size / stride / padding,
//                   bias + optional ReLU in the epilogue.  M = N*OH*OW output pixels, N = Cout,
//                   K = kh*kw*Cin in (kh, kw, ci) order, weights [Cout][kh][kw][Cin].
//                   Block tile 64 x 64 x 32, four waves, wave w owns rows 16w..16w+15 of the tile
//                   and all 64 columns as four independent 16x16 accumulators (the 16x16x4 form
//                   has a 40-cycle dependent latency against a 32-cycle issue interval).  No
//                   split-K and no atomics: every output element is ONE chain over k = 0..K-1, so
//                   an image's result does not depend on what else is in the batch.  K is padded
//                   to the tile with zeros formed in registers (fma(0, 0, acc) == acc), never by
//                   reading past a row; rows past M and padding taps are zeros the same way.
//                   LDS tiles are [row][k] with a 34-float row stride: the operand read of lane l
//                   (row l & 15, k = l >> 4) then hits bank (2 row + k) mod 32 — all 32 lanes of a
//                   ds_read_b32 group on distinct banks — and rows stay 8-byte aligned for the
//                   loader's ds_write_b64.
//   prep / maxpool  uint8 -> ScalingLayer'd fp32 NHWC (so the convs' zero padding is zero in
//                   scaled units), MaxPool2d(3, 2) on NHWC fp32.
//   vd_lpips_layer  one tap's distance: unit-normalise both feature vectors per pixel, lin-weighted
//                   squared difference, mean over pixels.  One wave per pixel (fp32 butterfly sums
//                   over the channels), fp64 across pixels in a fixed order: per-wave, per-block
//                   (workspace partials), then one thread per pair — deterministic, no atomics.
//   vd_lpips_pairs  the whole metric for [videos][frames] uint8 frames: features once per frame,
//                   every interior frame used by two pairs.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int BM = 64, BN = 64, BK = 32;
constexpr int LDT = 34;  // LDS row stride in floats (see the header comment)

struct ConvArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  int H, W, Cin, Cout, KW, stride, pad, OH, OW;
  int M, K, relu;
};

template <int VEC>
struct Vec;
template <>
struct Vec<4> {
  typedef f32x4 type;
};
template <>
struct Vec<1> {
  typedef float type;
};

template <int VEC>
__device__ __forceinline__ void lds_put(float* dst, const typename Vec<VEC>::type& v);
template <>
__device__ __forceinline__ void lds_put<4>(float* dst, const f32x4& v) {
  typedef float __attribute__((ext_vector_type(2))) f2;
  *(f2*)dst = f2{v[0], v[1]};
  *(f2*)(dst + 2) = f2{v[2], v[3]};
}
template <>
__device__ __forceinline__ void lds_put<1>(float* dst, const float& v) {
  *dst = v;
}

// VEC = 4: Cin % 4 == 0, 16-byte loads of four consecutive ci of one tap.  VEC = 1: any Cin
// (used for Cin == 3), scalar loads.
template <int VEC>
__global__ __launch_bounds__(NT) void conv_f32_kernel(ConvArgs p) {
  typedef typename Vec<VEC>::type vec_t;
  constexpr int KV = BK / VEC;   // loader columns (k vectors per tile row)
  constexpr int RPP = NT / KV;   // tile rows per loader pass
  constexpr int NP = BM / RPP;   // loader passes (BM == BN: the same for both tiles)
  __shared__ __attribute__((aligned(16))) float As[BM * LDT];
  __shared__ __attribute__((aligned(16))) float Bs[BN * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int kv = tid % KV, r0 = tid / KV;

  // this thread's tile rows: image base offset and the top-left input coordinate of the window
  int xoff[NP], ih0[NP], iw0[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int m = m0 + r0 + i * RPP;
    if (m < p.M) {
      const int ow = m % p.OW, t = m / p.OW, oh = t % p.OH, n = t / p.OH;
      xoff[i] = n * p.H * p.W * p.Cin;
      ih0[i] = oh * p.stride - p.pad;
      iw0[i] = ow * p.stride - p.pad;
    } else {  // a row past M: every tap fails the bounds test below and loads nothing
      xoff[i] = 0;
      ih0[i] = iw0[i] = -0x40000000;
    }
  }

  vec_t ra[NP], rb[NP];
  auto fetch = [&](int kt) {
    const int kg = kt * BK + kv * VEC;
    const bool kok = kg < p.K;  // VEC = 4: K % 4 == 0, so the whole vector is in or out
    const int ci = kg % p.Cin, t = kg / p.Cin, kw = t % p.KW, kh = t / p.KW;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int ih = ih0[i] + kh, iw = iw0[i] + kw;
      const bool ok = kok && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      vec_t v = {};
      if (ok) v = *(const vec_t*)(p.x + xoff[i] + (ih * p.W + iw) * p.Cin + ci);
      ra[i] = v;
      vec_t u = {};
      if (kok) u = *(const vec_t*)(p.w + (int64_t)(n0 + r0 + i * RPP) * p.K + kg);
      rb[i] = u;
    }
  };

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkt = (p.K + BK - 1) / BK;
  const int frow = lane & 15, fk = lane >> 4;
  fetch(0);
  for (int kt = 0; kt < nkt; ++kt) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      lds_put<VEC>(As + (r0 + i * RPP) * LDT + kv * VEC, ra[i]);
      lds_put<VEC>(Bs + (r0 + i * RPP) * LDT + kv * VEC, rb[i]);
    }
    __syncthreads();
    if (kt + 1 < nkt) fetch(kt + 1);  // the next tile's global loads fly under this tile's MFMAs
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      const float a = As[(wave * 16 + frow) * LDT + kk * 4 + fk];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float b = Bs[(j * 16 + frow) * LDT + kk * 4 + fk];
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // C/D map of the 16x16 forms: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = n0 + j * 16 + frow;
    const float bv = p.bias ? p.bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wave * 16 + fk * 4 + r;
      if (m < p.M) {
        float v = acc[j][r] + bv;
        if (p.relu) v = fmaxf(v, 0.f);
        p.y[(int64_t)m * p.Cout + co] = v;
      }
    }
  }
}

// uint8 [N][H][W][3] -> ScalingLayer(2 u / 255 - 1) fp32, same layout.  Formed in fp64 and
// rounded once, so the only fp32 quantities in it are shift and scale themselves.
__global__ __launch_bounds__(NT) void lpips_prep_kernel(const uint8_t* __restrict__ u, int64_t total,
                                                        const float* __restrict__ shift,
                                                        const float* __restrict__ scale, float* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int c = (int)(i % 3);
    const double v = 2.0 * ((double)u[i] / 255.0) - 1.0;
    y[i] = (float)((v - (double)shift[c]) / (double)scale[c]);
  }
}

// MaxPool2d(3, 2), no padding, floor mode, NHWC fp32, C % 4 == 0; one thread per four channels
__global__ __launch_bounds__(NT) void maxpool3s2_kernel(const float* __restrict__ x, int64_t total4, int H, int W,
                                                        int C4, int OH, int OW, float* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total4; i += (int64_t)gridDim.x * NT) {
    const int c = (int)(i % C4);
    int64_t t = i / C4;
    const int ow = (int)(t % OW);
    t /= OW;
    const int oh = (int)(t % OH);
    const int64_t n = t / OH;
    const f32x4* src = (const f32x4*)x + ((n * H + 2 * oh) * W + 2 * ow) * C4 + c;
    f32x4 m = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m = __builtin_elementwise_max(m, src[((int64_t)dy * W + dx) * C4]);
    ((f32x4*)y)[i] = m;
  }
}

constexpr int DIST_PB = 64;    // partial blocks per pair
constexpr int DIST_MAXC = 512;

// partial[pair][block] = sum over this block's pixels of sum_c lin[c] (na - nb)^2
__global__ __launch_bounds__(NT) void lpips_dist_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                        int pixels, int C, const float* __restrict__ lin,
                                                        double* __restrict__ partial) {
  const int pair = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nc = C / 64;
  const float* a0 = fa + (int64_t)pair * pixels * C;
  const float* b0 = fb + (int64_t)pair * pixels * C;
  float lw[DIST_MAXC / 64];
#pragma unroll
  for (int i = 0; i < DIST_MAXC / 64; ++i) lw[i] = i < nc ? lin[lane + 64 * i] : 0.f;
  double sum = 0.0;
  for (int px = blockIdx.x * (NT / 64) + wave; px < pixels; px += DIST_PB * (NT / 64)) {
    float va[DIST_MAXC / 64], vb[DIST_MAXC / 64];
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < DIST_MAXC / 64; ++i) {
      va[i] = vb[i] = 0.f;
      if (i < nc) {
        va[i] = a0[(int64_t)px * C + lane + 64 * i];
        vb[i] = b0[(int64_t)px * C + lane + 64 * i];
      }
      sa = fmaf(va[i], va[i], sa);
      sb = fmaf(vb[i], vb[i], sb);
    }
    const float da = sqrtf(wave_sum(sa)) + 1e-10f, db = sqrtf(wave_sum(sb)) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < DIST_MAXC / 64; ++i) {
      const float e = va[i] / da - vb[i] / db;
      d = fmaf(lw[i] * e, e, d);
    }
    sum += (double)wave_sum(d);
  }
  __shared__ double red[NT / 64];
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
    for (int i = 1; i < NT / 64; ++i) s += red[i];
    partial[(int64_t)pair * DIST_PB + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(NT) void lpips_dist_finalize(const double* __restrict__ partial, int pairs, int pixels,
                                                          int accumulate, double* __restrict__ out) {
  const int p = blockIdx.x * NT + threadIdx.x;
  if (p >= pairs) return;
  double s = 0.0;
  for (int i = 0; i < DIST_PB; ++i) s += partial[(int64_t)p * DIST_PB + i];
  s /= (double)pixels;
  out[p] = accumulate ? out[p] + s : s;
}

unsigned grid_for(int64_t n) {
  const int64_t b = (n + NT - 1) / NT;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

bool conv_shape_ok(int64_t N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0) return false;
  if (Cout % 64 != 0 || !(Cin % 4 == 0 || Cin == 3)) return false;
  if (H + 2 * pad < kh || W + 2 * pad < kw) return false;
  const int64_t OH = (H + 2 * pad - kh) / stride + 1, OW = (W + 2 * pad - kw) / stride + 1;
  // 32-bit element offsets inside the kernel
  return N * H * W * Cin < 0x7fffffffLL && N * OH * OW * Cout < 0x7fffffffLL && (int64_t)kh * kw * Cin < 0x7fffffffLL;
}

int conv_launch(const float* x, int64_t N, int H, int W, int Cin, const float* w, const float* bias, int Cout, int kh,
                int kw, int stride, int pad, int relu, float* y, hipStream_t s) {
  ConvArgs a;
  a.x = x; a.w = w; a.bias = bias; a.y = y;
  a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KW = kw; a.stride = stride; a.pad = pad;
  a.OH = (H + 2 * pad - kh) / stride + 1;
  a.OW = (W + 2 * pad - kw) / stride + 1;
  a.M = (int)(N * a.OH * a.OW);
  a.K = kh * kw * Cin;
  a.relu = relu;
  const dim3 grid((unsigned)((a.M + BM - 1) / BM), (unsigned)(Cout / BN));
  if (Cin % 4 == 0)
    hipLaunchKernelGGL(conv_f32_kernel<4>, grid, dim3(NT), 0, s, a);
  else
    hipLaunchKernelGGL(conv_f32_kernel<1>, grid, dim3(NT), 0, s, a);
  return vd_launch_status();
}

int dist_launch(const float* fa, const float* fb, int pairs, int pixels, int C, const float* lin, double* out,
                int accumulate, double* partial, hipStream_t s) {
  hipLaunchKernelGGL(lpips_dist_kernel, dim3(DIST_PB, (unsigned)pairs), dim3(NT), 0, s, fa, fb, pixels, C, lin,
                     partial);
  hipLaunchKernelGGL(lpips_dist_finalize, dim3(grid_for(pairs)), dim3(NT), 0, s, (const double*)partial, pairs,
                     pixels, accumulate, out);
  return vd_launch_status();
}

// AlexNet `features` as LPIPS slices it: {Cin, Cout, k, stride, pad}, a MaxPool2d(3, 2) before
// conv 2 and conv 3
constexpr int NCONV = 5;
constexpr int CONV[NCONV][5] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1},
                                {256, 256, 3, 1, 1}};

struct Sizes {
  int h[NCONV], w[NCONV];    // tap (ReLU output) sizes
  int ph[2], pw[2];          // pooled sizes after taps 1 and 2
};
bool lpips_sizes(int H, int W, Sizes& z) {
  if (H < 31 || W < 31) return false;
  z.h[0] = (H + 4 - 11) / 4 + 1; z.w[0] = (W + 4 - 11) / 4 + 1;
  z.ph[0] = (z.h[0] - 3) / 2 + 1; z.pw[0] = (z.w[0] - 3) / 2 + 1;
  z.h[1] = z.ph[0]; z.w[1] = z.pw[0];
  if (z.h[1] < 3 || z.w[1] < 3) return false;
  z.ph[1] = (z.h[1] - 3) / 2 + 1; z.pw[1] = (z.w[1] - 3) / 2 + 1;
  for (int l = 2; l < NCONV; ++l) { z.h[l] = z.ph[1]; z.w[l] = z.pw[1]; }
  return true;
}

// workspace of vd_lpips_pairs, in floats per image (every count is a multiple of 4 after the
// first, and the first is padded, so each buffer stays 16-byte aligned), then the fp64 partials
struct Layout {
  int64_t x0, tap[NCONV], pool[2], partial, bytes;
};
bool lpips_layout(int64_t images, int H, int W, Layout& L, Sizes& z) {
  if (images < 1 || !lpips_sizes(H, W, z)) return false;
  if (images * H * W * 3 >= 0x7fffffffLL || images * z.h[0] * z.w[0] * 64 >= 0x7fffffffLL) return false;
  int64_t off = 0;
  auto take = [&](int64_t floats) {
    const int64_t at = off;
    off += (floats + 3) / 4 * 4;
    return at;
  };
  L.x0 = take(images * H * W * 3);
  for (int l = 0; l < NCONV; ++l) {
    L.tap[l] = take(images * z.h[l] * z.w[l] * CONV[l][1]);
    if (l < 2) L.pool[l] = take(images * z.ph[l] * z.pw[l] * CONV[l][1]);
  }
  L.partial = off * 4;
  L.bytes = L.partial + images * DIST_PB * (int64_t)sizeof(double);
  return true;
}

}  // namespace

extern "C" int vd_conv2d_f32(const float* x, int64_t N, int32_t H, int32_t W, int32_t Cin, const float* w,
                             const float* bias, int32_t Cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                             int32_t relu, float* y, vd_stream_t stream) {
  VD_CHECK_ARG(x && w && y);
  VD_CHECK_ARG(conv_shape_ok(N, H, W, Cin, Cout, kh, kw, stride, pad));
  if (Cin % 4 == 0) VD_CHECK_ARG((((uintptr_t)x | (uintptr_t)w) & 15) == 0);
  return conv_launch(x, N, H, W, Cin, w, bias, Cout, kh, kw, stride, pad, relu, y, (hipStream_t)stream);
}

extern "C" int64_t vd_lpips_layer_workspace(int64_t pairs) {
  return pairs < 1 ? -1 : pairs * DIST_PB * (int64_t)sizeof(double);
}

extern "C" int vd_lpips_layer(const float* fa, const float* fb, int64_t pairs, int64_t pixels, int32_t C,
                              const float* lin, double* out, int32_t accumulate, void* workspace,
                              int64_t workspace_bytes, vd_stream_t stream) {
  VD_CHECK_ARG(fa && fb && lin && out && workspace);
  VD_CHECK_ARG(pairs >= 1 && pairs <= 65535 && pixels >= 1 && pixels < 0x7fffffffLL);
  VD_CHECK_ARG(C >= 64 && C % 64 == 0 && C <= DIST_MAXC);
  VD_CHECK_ARG(workspace_bytes >= pairs * DIST_PB * (int64_t)sizeof(double) && ((uintptr_t)workspace & 7) == 0);
  return dist_launch(fa, fb, (int)pairs, (int)pixels, C, lin, out, accumulate, (double*)workspace,
                     (hipStream_t)stream);
}

extern "C" int64_t vd_lpips_workspace(int64_t images, int32_t H, int32_t W) {
  Layout L;
  Sizes z;
  return lpips_layout(images, H, W, L, z) ? L.bytes : -1;
}

extern "C" int vd_lpips_pairs(const void* frames_u8, int64_t videos, int32_t frames, int32_t H, int32_t W,
                              const float* params, double* out, void* workspace, int64_t workspace_bytes,
                              vd_stream_t stream) {
  VD_CHECK_ARG(frames_u8 && params && out && workspace);
  VD_CHECK_ARG(videos >= 1 && frames >= 2 && frames <= 65536 && videos < 0x7fffffffLL / frames);
  VD_CHECK_ARG((((uintptr_t)params | (uintptr_t)workspace) & 15) == 0);
  const int64_t images = videos * frames;
  Layout L;
  Sizes z;
  VD_CHECK_ARG(lpips_layout(images, H, W, L, z) && workspace_bytes >= L.bytes);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  double* partial = (double*)((char*)workspace + L.partial);

  // the parameter blob (include/vdiff.h): weights, biases, lin vectors, shift, scale
  const float* wp[NCONV];
  const float* bp[NCONV];
  const float* lp[NCONV];
  const float* q = params;
  for (int l = 0; l < NCONV; ++l) { wp[l] = q; q += (int64_t)CONV[l][1] * CONV[l][2] * CONV[l][2] * CONV[l][0]; }
  for (int l = 0; l < NCONV; ++l) { bp[l] = q; q += CONV[l][1]; }
  for (int l = 0; l < NCONV; ++l) { lp[l] = q; q += CONV[l][1]; }
  const float* shift = q;
  const float* scale = q + 3;

  const int64_t n0 = images * H * W * 3;
  hipLaunchKernelGGL(lpips_prep_kernel, dim3(grid_for(n0)), dim3(NT), 0, s, (const uint8_t*)frames_u8, n0, shift,
                     scale, ws + L.x0);
  const float* in = ws + L.x0;
  int ih = H, iw = W;
  for (int l = 0; l < NCONV; ++l) {
    float* tap = ws + L.tap[l];
    const int rc = conv_launch(in, images, ih, iw, CONV[l][0], wp[l], bp[l], CONV[l][1], CONV[l][2], CONV[l][2],
                               CONV[l][3], CONV[l][4], 1, tap, s);
    if (rc != VD_OK) return rc;
    // this tap's distance of every pair (f, f+1) of each video, summed into out over the taps
    const int64_t pixels = (int64_t)z.h[l] * z.w[l], fstride = pixels * CONV[l][1];
    for (int64_t v = 0; v < videos; ++v) {
      const float* fa = tap + v * frames * fstride;
      const int rd = dist_launch(fa, fa + fstride, frames - 1, (int)pixels, CONV[l][1], lp[l],
                                 out + v * (frames - 1), l > 0, partial, s);
      if (rd != VD_OK) return rd;
    }
    in = tap;
    ih = z.h[l]; iw = z.w[l];
    if (l < 2) {
      float* pl = ws + L.pool[l];
      const int64_t total4 = images * z.ph[l] * z.pw[l] * (CONV[l][1] / 4);
      hipLaunchKernelGGL(maxpool3s2_kernel, dim3(grid_for(total4)), dim3(NT), 0, s, (const float*)tap, total4, ih,
                         iw, CONV[l][1] / 4, z.ph[l], z.pw[l], pl);
      in = pl;
      ih = z.ph[l]; iw = z.pw[l];
    }
  }
  return vd_launch_status();
}
