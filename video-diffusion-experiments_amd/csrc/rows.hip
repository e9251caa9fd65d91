// Elementwise row ops over bf16 NHWC rows: the pieces of diffusers' module-level
// forward that the fused fast path never materialises — residual adds
// (`attn_output + hidden_states`, `hidden_states + residual`), the ResnetBlock2D time
// embedding broadcast (`h + temb[:, :, None, None]`), SinusoidalPositionalEmbedding
// (`x + pe[:, :S]`), `repeat_interleave(num_frames)`, `torch.cat([x, skip], 1)`
// (column slices), `nn.SiLU`, and Upsample2D's `F.interpolate(scale_factor=2,
// mode="nearest")`.  They run when a caller drives the modules one by one (the
// reference's forward-hook tracing, experiments/03_trace_forward_pass.py:105-113 via
// utils/forward_tracer.py:177-206, or a direct motion_modules[i](x, num_frames=F)
// call, 03:182) — so every module's __call__ sees diffusers-shaped tensors while
// all arithmetic stays on HIP kernels.  HBM-bound: 16-byte chunks, one per thread.
#include "common.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ void load8_any(const void* p, int is_f32, float* f) {
  if (is_f32) {
    const float4 a = *(const float4*)p, b = *((const float4*)p + 1);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    unpack8(*(const uint4*)p, f);
  }
}

// op 0: out[r] = (x ? x[r] : 0) + y[(r / y_div) % y_period]     (y bf16 or fp32)
// op 1: out[r] = silu(x[r])
// op 3: out[r] = x[r] * *y                                        (y one fp32 on the device)
// (op 2 is freeu_filter_kernel, ops 4 and 5 win_gather_kernel / win_merge_kernel, op 7 ctrl_add_kernel,
// op 8 sparse_cond_kernel, op 9 prompt_lerp_kernel below)
__global__ void rows_eltwise_kernel(int op, const bf16_t* x, int64_t ldx, const void* y, int64_t ldy, int y_f32,
                                    int64_t y_div, int64_t y_period, int64_t rows, int64_t C, bf16_t* out,
                                    int64_t ldo) {
  const int64_t cpr = C / 8;
  const int64_t total = rows * cpr;
  const float g = op == VD_ROWS_SCALE ? *(const float*)y : 1.0f;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t r = i / cpr;
    const int64_t c = (i - r * cpr) * 8;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (x) unpack8(*(const uint4*)(x + r * ldx + c), v);
    if (op == VD_ROWS_SCALE) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= g;
    } else if (op == 0) {
      const int64_t yr = (r / y_div) % y_period;
      float w[8];
      load8_any(y_f32 ? (const void*)((const float*)y + yr * ldy + c) : (const void*)((const bf16_t*)y + yr * ldy + c),
                y_f32, w);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += w[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = silu_f(v[j]);
    }
    *(uint4*)(out + r * ldo + c) = pack8(v);
  }
}

// out row (n, y, x) of the 2h x 2w grid <- in row (n, y/2, x/2)
__global__ void upsample2x_kernel(const bf16_t* x, int64_t ldx, int64_t n_img, int64_t h, int64_t w, int64_t C,
                                  bf16_t* out, int64_t ldo) {
  const int64_t cpr = C / 8;
  const int64_t total = n_img * 4 * h * w * cpr;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t r = i / cpr;
    const int64_t c = (i - r * cpr) * 8;
    const int64_t ox = r % (2 * w), oy = (r / (2 * w)) % (2 * h), n = r / (4 * h * w);
    const int64_t src = (n * h + oy / 2) * w + ox / 2;
    *(uint4*)(out + r * ldo + c) = *(const uint4*)(x + src * ldx + c);
  }
}

// op 2, FreeU's fourier_filter(threshold = 1): per (image, channel) plane of H x W pixels, with
// th = 2 pi h / H and tw = 2 pi w / W,
//   out = x + (s - 1) / (H W) * (A + B cos th + C sin th + D cos tw + E sin tw
//                                  + P cos(th + tw) + Q sin(th + tw)),
// A .. Q the plane's sums of x times the same seven factors (the four FFT bins k_h, k_w in
// {-1, 0} that diffusers' 2 x 2 mask scales, written out; include/vdiff.h).
// One workgroup per (image, slab of n8 8-channel chunks): thread t owns chunk t % n8 (a pixel
// row's n8 * 16 bytes are contiguous over adjacent threads) and pixel lane t / n8 of FU_L, i.e.
// pixels lane, lane + FU_L, ...  The summation order of a plane is a function of (H, W) alone:
// a lane adds its pixels in ascending order, the FU_L lanes are combined as a balanced tree over
// the lane index bits, lowest first — wave shuffles for the bits inside a wave, LDS for the
// bits that select the wave — and a + b == b + a makes the butterfly's two sides equal.  So the
// slab width n8 (chosen from the grid size, i.e. from n_img) and the image's index change no bit.
// KEEP: planes of <= FU_L * FU_KEEP pixels (every UNet shape) stay in registers between the two
// passes; larger planes are read again.
constexpr int FU_L = 32, FU_KEEP = 8, FU_NS = 7;
constexpr int FU_RED = 4 * 8 * FU_NS * 8;  // floats: [wave][chunk][sum][channel]

struct FuTw {
  float ch, sh, cw, sw, cp, sp;
};
__device__ __forceinline__ FuTw fu_twiddle(const float2* tw, int p, int H, int W) {
  const int h = p / W, w = p - h * W;
  const float2 a = tw[h], b = tw[H + w];
  return {a.x, a.y, b.x, b.y, a.x * b.x - a.y * b.y, a.y * b.x + a.x * b.y};
}
__device__ __forceinline__ void fu_accum(float (&acc)[FU_NS][8], const uint4& u, const FuTw& t) {
  float f[8];
  unpack8(u, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc[0][e] += f[e];
    acc[1][e] = fmaf(f[e], t.ch, acc[1][e]);
    acc[2][e] = fmaf(f[e], t.sh, acc[2][e]);
    acc[3][e] = fmaf(f[e], t.cw, acc[3][e]);
    acc[4][e] = fmaf(f[e], t.sw, acc[4][e]);
    acc[5][e] = fmaf(f[e], t.cp, acc[5][e]);
    acc[6][e] = fmaf(f[e], t.sp, acc[6][e]);
  }
}
__device__ __forceinline__ uint4 fu_apply(const float (&acc)[FU_NS][8], const uint4& u, const FuTw& t, float k) {
  float f[8];
  unpack8(u, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float c = fmaf(acc[1][e], t.ch, acc[0][e]);
    c = fmaf(acc[2][e], t.sh, c);
    c = fmaf(acc[3][e], t.cw, c);
    c = fmaf(acc[4][e], t.sw, c);
    c = fmaf(acc[5][e], t.cp, c);
    c = fmaf(acc[6][e], t.sp, c);
    f[e] = fmaf(k, c, f[e]);
  }
  return pack8(f);
}

template <bool KEEP>
__global__ __launch_bounds__(NT) void freeu_filter_kernel(const bf16_t* x, int64_t ldx, const float* s_dev, int H,
                                                          int W, int n8, int nslab, bf16_t* out, int64_t ldo) {
  extern __shared__ __attribute__((aligned(16))) float fu_smem[];
  float* red = fu_smem;                      // the waves' partial sums
  float2* tw = (float2*)(fu_smem + FU_RED);  // (cos, sin) of 2 pi i / H, then of 2 pi j / W
  const int t = threadIdx.x, pix = H * W;
  for (int i = t; i < H + W; i += blockDim.x) {
    // sin / cos of pi * a, a in [0, 2): no large angle is ever reduced
    const float a = i < H ? 2.0f * (float)i / (float)H : 2.0f * (float)(i - H) / (float)W;
    float sn, cs;
    sincospif(a, &sn, &cs);
    tw[i] = make_float2(cs, sn);
  }
  __syncthreads();
  const int c8 = t % n8, lane = t / n8;
  const bool act = lane < FU_L;  // n8 == 1 runs one wave, its upper half idle
  const int img = blockIdx.x / nslab, slab = blockIdx.x % nslab;
  const int64_t c = ((int64_t)slab * n8 + c8) * 8;
  const bf16_t* xp = x + (int64_t)img * pix * ldx + c;
  bf16_t* dst = out + (int64_t)img * pix * ldo + c;

  float acc[FU_NS][8];
#pragma unroll
  for (int j = 0; j < FU_NS; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
  uint4 v[KEEP ? FU_KEEP : 1];
  if (KEEP) {
#pragma unroll
    for (int k = 0; k < FU_KEEP; ++k) {
      const int p = lane + k * FU_L;
      v[k] = make_uint4(0, 0, 0, 0);
      if (act && p < pix) v[k] = *(const uint4*)(xp + (int64_t)p * ldx);
    }
#pragma unroll
    for (int k = 0; k < FU_KEEP; ++k) {
      const int p = lane + k * FU_L;
      if (act && p < pix) fu_accum(acc, v[k], fu_twiddle(tw, p, H, W));
    }
  } else if (act) {
    for (int p = lane; p < pix; p += FU_L) fu_accum(acc, *(const uint4*)(xp + (int64_t)p * ldx), fu_twiddle(tw, p, H, W));
  }

  // lane bits inside the wave: threads t and t ^ o hold the same chunk, lanes that differ in one bit
  for (int o = n8; o < 64; o <<= 1) {
#pragma unroll
    for (int j = 0; j < FU_NS; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][e] += __shfl_xor(acc[j][e], o, 64);
  }
  // lane bits that select the wave (n8 = 4: two waves, n8 = 8: four)
  const int nw = blockDim.x / 64;
  if (nw > 1) {
    const int wv = t / 64;
    if ((t & 63) < n8) {
#pragma unroll
      for (int j = 0; j < FU_NS; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[((wv * n8 + c8) * FU_NS + j) * 8 + e] = acc[j][e];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FU_NS; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int q = (c8 * FU_NS + j) * 8 + e, ws = n8 * FU_NS * 8;
        const float a = red[q] + red[ws + q];
        acc[j][e] = nw == 2 ? a : a + (red[2 * ws + q] + red[3 * ws + q]);
      }
  }
  if (!act) return;

  const float k = (*s_dev - 1.0f) / (float)pix;
  if (KEEP) {
#pragma unroll
    for (int kk = 0; kk < FU_KEEP; ++kk) {
      const int p = lane + kk * FU_L;
      if (p < pix) *(uint4*)(dst + (int64_t)p * ldo) = fu_apply(acc, v[kk], fu_twiddle(tw, p, H, W), k);
    }
  } else {
    for (int p = lane; p < pix; p += FU_L)
      *(uint4*)(dst + (int64_t)p * ldo) = fu_apply(acc, *(const uint4*)(xp + (int64_t)p * ldx), fu_twiddle(tw, p, H, W), k);
  }
}

// Ops 4 and 5, FreeNoise's sliding windows over the frames of (video b, frame f, position p) rows
// (diffusers' FreeNoiseTransformerBlock; include/vdiff.h has the geometry).  Window w < nReg
// starts at frame w * s, the tail window (index nReg, when there is one) at F - L.
// One workgroup works inside one frame: the window list and the normaliser are wave-uniform
// (scalar registers), and a thread walks the frame's hw * C / 8 16-byte chunks with a
// (row, chunk) pair advanced by the host's (dr, dc) = divmod(gridDim.y * NT, C / 8): one 32-bit
// division per thread, none per element.
struct WinGeo {
  int F, L, s, nReg, nW;  // frames, context length, stride, regular windows, all windows
  int hw, cpr;            // positions per frame, 16-byte chunks per row
  int dr, dc;             // divmod(gridDim.y * NT, cpr)
};

struct WinPos {
  int r, c;
  __device__ __forceinline__ WinPos(const WinGeo& g) {
    const unsigned i = blockIdx.y * NT + threadIdx.x;
    r = (int)(i / (unsigned)g.cpr);
    c = (int)(i - (unsigned)r * (unsigned)g.cpr);
  }
  __device__ __forceinline__ void next(const WinGeo& g) {
    r += g.dr;
    c += g.dc;
    if (c >= g.cpr) {
      c -= g.cpr;
      ++r;
    }
  }
};

// op 4: out frame (b, w, j) <- x frame (b, start_w + j); blockIdx.x = (b * nW + w) * L + j
__global__ __launch_bounds__(NT) void win_gather_kernel(const bf16_t* x, int64_t ldx, WinGeo g, bf16_t* out,
                                                        int64_t ldo) {
  const int fo = blockIdx.x, j = fo % g.L, bw = fo / g.L, w = bw % g.nW, b = bw / g.nW;
  const int start = w < g.nReg ? w * g.s : g.F - g.L;
  const bf16_t* src = x + ((int64_t)b * g.F + start + j) * g.hw * ldx;
  bf16_t* dst = out + (int64_t)fo * g.hw * ldo;
  for (WinPos p(g); p.r < g.hw; p.next(g))
    *(uint4*)(dst + (int64_t)p.r * ldo + p.c * 8) = *(const uint4*)(src + (int64_t)p.r * ldx + p.c * 8);
}

// op 5: out frame (b, f) <- the weighted mean of the regular windows that hold f, ascending w, or
// the tail window's frame where no regular window reaches; blockIdx.x = b * F + f.  Four
// windows' loads are in flight before the first is consumed (the default L = 16, s = 4 has at
// most four per frame); the order of the fp32 sum is that of w whatever the grouping.
constexpr int WIN_G = 4;
__global__ __launch_bounds__(NT) void win_merge_kernel(const bf16_t* x, int64_t ldx, const float* wt, WinGeo g,
                                                       bf16_t* out, int64_t ldo) {
  const int b = blockIdx.x / g.F, f = blockIdx.x - b * g.F;
  bf16_t* dst = out + (int64_t)blockIdx.x * g.hw * ldo;
  const int64_t vid = (int64_t)b * g.nW;  // the video's first window
  if (f >= (g.nReg - 1) * g.s + g.L) {    // a tail frame: the tail window's value as it is
    const bf16_t* src = x + ((vid + g.nReg) * g.L + (f - (g.F - g.L))) * g.hw * ldx;
    for (WinPos p(g); p.r < g.hw; p.next(g))
      *(uint4*)(dst + (int64_t)p.r * ldo + p.c * 8) = *(const uint4*)(src + (int64_t)p.r * ldx + p.c * 8);
    return;
  }
  const int w_lo = f < g.L ? 0 : (f - g.L) / g.s + 1;
  const int w_hi = min(f / g.s, g.nReg - 1);
  float den = 0.f;
  for (int w = w_lo; w <= w_hi; ++w) den += wt[f - w * g.s];
  for (WinPos p(g); p.r < g.hw; p.next(g)) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int w0 = w_lo; w0 <= w_hi; w0 += WIN_G) {
      uint4 v[WIN_G];
#pragma unroll
      for (int k = 0; k < WIN_G; ++k) {
        const int w = w0 + k, j = f - w * g.s;
        if (w <= w_hi) v[k] = *(const uint4*)(x + (((vid + w) * g.L + j) * g.hw + p.r) * ldx + p.c * 8);
      }
#pragma unroll
      for (int k = 0; k < WIN_G; ++k) {
        const int w = w0 + k;
        if (w <= w_hi) {
          const float a = wt[f - w * g.s];
          float e[8];
          unpack8(v[k], e);
#pragma unroll
          for (int q = 0; q < 8; ++q) acc[q] = fmaf(a, e[q], acc[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = acc[q] / den;
    *(uint4*)(dst + (int64_t)p.r * ldo + p.c * 8) = pack8(acc);
  }
}

// op 7, ControlNet's residual injection: out[r][c] += s * x[r][c], s one entry of the fp32 table
// behind the control block's 4-float header, picked by the device step index in the header's
// first word (clamped to the table) and the column the op word carries (include/vdiff.h).  Every
// thread reads the same two words, so step, scale and data are all read inside the launch.
__global__ __launch_bounds__(NT) void ctrl_add_kernel(const bf16_t* x, int64_t ldx, const float* blk, int ldy, int col,
                                                      int period, int64_t rows, int64_t C, bf16_t* out, int64_t ldo) {
  const int step = min(max(*(const int*)blk, 0), period - 1);
  const float s = blk[4 + (int64_t)step * ldy + col];
  const int64_t cpr = C / 8;
  const int64_t total = rows * cpr;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t r = i / cpr;
    const int64_t c = (i - r * cpr) * 8;
    float z[8], v[8];
    unpack8(*(const uint4*)(x + r * ldx + c), z);
    unpack8(*(const uint4*)(out + r * ldo + c), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaf(s, z[j], v[j]);
    *(uint4*)(out + r * ldo + c) = pack8(v);
  }
}

// op 8, SparseCtrl's condition rows: out row (b, f, p) <- key frame k* of video b, k* the LARGEST k
// with idx[k] == f, its cc channels as they are, bf16 1.0 in column cc (the conditioning mask), +0
// above; a frame no index names is +0 in all 8 columns (include/vdiff.h).  A gather: every workgroup
// first turns the K indices into a frame -> k* table in LDS (thread f scans the indices in ascending
// k, so the last assignment wins whatever the launch geometry; an index outside [0, F) matches no
// thread), then one lane per output row does one 16-byte load (conditioned frames only) and one
// 16-byte store.  No scatter, no atomics; every output element is written.
constexpr int SPARSE_MAX = 256;  // the longest F and K: F <= NT fills the table in one pass
__global__ __launch_bounds__(NT) void sparse_cond_kernel(const bf16_t* x, int64_t ldx, const int* idx, int K, int F,
                                                         int64_t hw, int cc, int64_t rows, bf16_t* out, int64_t ldo) {
  __shared__ int kof[SPARSE_MAX];
  for (int f = threadIdx.x; f < F; f += NT) {
    int ks = -1;
    for (int k = 0; k < K; ++k)
      if (idx[k] == f) ks = k;
    kof[f] = ks;
  }
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x; r < rows; r += (int64_t)gridDim.x * NT) {
    const int64_t bf = r / hw, p = r - bf * hw, b = bf / F;
    const int ks = kof[(int)(bf - b * F)];
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ks >= 0) {
      const uint4 u = *(const uint4*)(x + ((b * K + ks) * hw + p) * ldx);
      const uint32_t in[4] = {u.x, u.y, u.z, u.w};
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // columns 2j (low half) and 2j + 1 (high half)
        const uint32_t lo = 2 * j < cc ? (in[j] & 0xffffu) : (2 * j == cc ? 0x3f80u : 0u);
        const uint32_t hi = 2 * j + 1 < cc ? (in[j] & 0xffff0000u) : (2 * j + 1 == cc ? 0x3f800000u : 0u);
        o[j] = lo | hi;
      }
      v = make_uint4(o[0], o[1], o[2], o[3]);
    }
    *(uint4*)(out + r * ldo) = v;
  }
}

// op 9, FreeNoise prompt travel: out row (b, f, l) <- the key prompts' token row l, interpolated
// linearly between the two key frames around f (include/vdiff.h).  Every workgroup first copies the
// K indices into LDS and turns them into a frame -> (k, exact) table and a frame -> weight table there
// (thread f scans the indices in ascending k and keeps the last k with idx[k] <= f: at most K <= 256
// broadcast LDS reads, once per workgroup), then one lane per 16-byte chunk does
// one load and a copy on a key frame, two loads and eight fused multiply-adds elsewhere.  k and
// k + 1 are clamped into [0, K - 1], so a table that breaks the contract reads inside x.
constexpr int PROMPT_MAX = 256;  // the longest F and K: F <= NT fills the tables in one pass
__global__ __launch_bounds__(NT) void prompt_lerp_kernel(const bf16_t* x, int64_t ldx, const int* idx, int K, int F,
                                                         int64_t L, int64_t rows, int64_t C, bf16_t* out,
                                                         int64_t ldo) {
  __shared__ int kof[PROMPT_MAX];    // 2 * k + (f == idx[k])
  __shared__ float wof[PROMPT_MAX];  // float(f - idx[k]) / float(idx[k + 1] - idx[k])
  __shared__ int sidx[PROMPT_MAX];   // the K indices: one global load each, the scans below read LDS
  for (int k = threadIdx.x; k < K; k += NT) sidx[k] = idx[k];
  __syncthreads();
  for (int f = threadIdx.x; f < F; f += NT) {
    int ks = 0;
    for (int k = 0; k < K; ++k)
      if (sidx[k] <= f) ks = k;
    const int lo = sidx[ks], hi = sidx[min(ks + 1, K - 1)];
    kof[f] = 2 * ks + (lo == f ? 1 : 0);
    wof[f] = (float)(f - lo) / (float)(hi - lo);
  }
  __syncthreads();
  const int64_t cpr = C / 8;
  const int64_t total = rows * cpr;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t r = i / cpr;
    const int64_t c = (i - r * cpr) * 8;
    const int64_t bf = r / L, l = r - bf * L, b = bf / F;
    const int f = (int)(bf - b * F);
    const int ke = kof[f], ka = ke >> 1, kb = min(ka + 1, K - 1);
    const uint4 ua = *(const uint4*)(x + ((b * K + ka) * L + l) * ldx + c);
    uint4 v = ua;
    if (!(ke & 1)) {
      const uint4 ub = *(const uint4*)(x + ((b * K + kb) * L + l) * ldx + c);
      const float w = wof[f], u = 1.0f - w;
      float ea[8], eb[8];
      unpack8(ua, ea);
      unpack8(ub, eb);
#pragma unroll
      for (int j = 0; j < 8; ++j) ea[j] = fmaf(w, eb[j], u * ea[j]);
      v = pack8(ea);
    }
    *(uint4*)(out + r * ldo + c) = v;
  }
}

unsigned grid_for(int64_t total) {
  const int64_t b = (total + NT - 1) / NT;
  return (unsigned)(b < 16384 ? (b > 0 ? b : 1) : 16384);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// true for an address inside a device allocation (no launch, no synchronisation; a failed query
// — a host address, no device — leaves no sticky error behind)
inline bool on_device(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}

}  // namespace

// op 6, FreeInit's spectral low-pass: fp32 volumes and rules of its own (spectral.hip)
namespace vdrows __attribute__((visibility("hidden"))) {
int spectral_launch(int32_t pass, const void* x, int64_t ldx, const void* y, int64_t ldy, int32_t y_f32, int64_t H,
                    int64_t F, int64_t rows, int64_t W, void* out, int64_t ldo, vd_stream_t stream);
}

extern "C" int vd_rows_eltwise(int32_t op, const void* x, int64_t ldx, const void* y, int64_t ldy, int32_t y_f32,
                               int64_t y_div, int64_t y_period, int64_t rows, int64_t C, void* out, int64_t ldo,
                               vd_stream_t stream) {
  // op 6 carries its pass above the low byte (VD_ROWS_SPEC_PASS); none of the bf16 rules below apply
  if (op >= 0 && (op & 0xff) == VD_ROWS_SPECTRAL)
    return vdrows::spectral_launch(op >> 8, x, ldx, y, ldy, y_f32, y_div, y_period, rows, C, out, ldo, stream);
  // op 7 carries its table column above the low byte (VD_ROWS_CTRL_COL); out is read and written
  if (op >= 0 && (op & 0xff) == VD_ROWS_CTRL_ADD) {
    const int32_t col = op >> 8;  // a bit above the column byte makes col > 255, past any ldy <= 64
    VD_CHECK_ARG(x && y && out && al16(x) && al16(y) && al16(out) && x != out && y_f32 == 1);
    VD_CHECK_ARG(ldy >= 1 && ldy <= 64 && col < ldy && y_period >= 1 && y_period <= 0x7fffffff);
    VD_CHECK_ARG(rows > 0 && C > 0 && C % 8 == 0 && ldx % 8 == 0 && ldo % 8 == 0 && ldx >= C && ldo >= C);
    // the control block must be DEVICE memory: every thread reads the step word through y before
    // any bound is known, and before this op existed a plain op 7 was refused whatever its operands
    VD_CHECK_ARG(on_device(y));
    hipLaunchKernelGGL(ctrl_add_kernel, dim3(grid_for(rows * (C / 8))), dim3(NT), 0, (hipStream_t)stream,
                       (const bf16_t*)x, ldx, (const float*)y, (int)ldy, (int)col, (int)y_period, rows, C,
                       (bf16_t*)out, ldo);
    return vd_launch_status();
  }
  // op 8 carries its channel count above the low byte (VD_ROWS_SPARSE_CH); a plain op 8 carries 0 and
  // stays refused, a bit above the channel byte makes cc > 7
  if (op >= 0 && (op & 0xff) == VD_ROWS_SPARSE_COND) {
    const int32_t cc = op >> 8;
    const int64_t F = y_period, hw = y_div, K = ldy;
    VD_CHECK_ARG(cc >= 1 && cc <= 7 && C == 8);
    VD_CHECK_ARG(K >= 1 && K <= SPARSE_MAX && F >= 1 && F <= SPARSE_MAX && hw >= 1 && rows > 0 && hw <= rows);
    VD_CHECK_ARG(rows % (F * hw) == 0);
    VD_CHECK_ARG(x && out && al16(x) && al16(out) && x != out);
    VD_CHECK_ARG(ldx >= 8 && ldo >= 8 && ldx % 8 == 0 && ldo % 8 == 0);
    // the K indices must be DEVICE memory, as op 7's control block: every workgroup reads them
    VD_CHECK_ARG(y && ((uintptr_t)y & 3) == 0 && y_f32 == 1 && on_device(y));
    hipLaunchKernelGGL(sparse_cond_kernel, dim3(grid_for(rows)), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)x,
                       ldx, (const int*)y, (int)K, (int)F, hw, (int)cc, rows, (bf16_t*)out, ldo);
    return vd_launch_status();
  }
  // op 9 carries nothing above the low byte; the K indices are DEVICE memory, as op 8's
  if (op >= 0 && (op & 0xff) == VD_ROWS_PROMPT_LERP) {
    const int64_t F = y_period, L = y_div, K = ldy;
    VD_CHECK_ARG((op >> 8) == 0 && C > 0 && C % 8 == 0);
    VD_CHECK_ARG(K >= 1 && K <= PROMPT_MAX && F >= 1 && F <= PROMPT_MAX && L >= 1 && rows > 0 && L <= rows);
    VD_CHECK_ARG(rows % (F * L) == 0);
    VD_CHECK_ARG(x && out && al16(x) && al16(out) && x != out);
    VD_CHECK_ARG(ldx >= C && ldo >= C && ldx % 8 == 0 && ldo % 8 == 0);
    VD_CHECK_ARG(y && ((uintptr_t)y & 3) == 0 && y_f32 == 1 && on_device(y));
    hipLaunchKernelGGL(prompt_lerp_kernel, dim3(grid_for(rows * (C / 8))), dim3(NT), 0, (hipStream_t)stream,
                       (const bf16_t*)x, ldx, (const int*)y, (int)K, (int)F, L, rows, C, (bf16_t*)out, ldo);
    return vd_launch_status();
  }
  // ops 4 and 5 carry the window stride above the low byte (VD_ROWS_WIN_STRIDE); no other op does
  const int32_t win_s = op >> 8;
  const bool win = op >= 0 && ((op & 0xff) == VD_ROWS_WIN_GATHER || (op & 0xff) == VD_ROWS_WIN_MERGE);
  if (win) op &= 0xff;
  VD_CHECK_ARG(op >= VD_ROWS_ADD && op <= VD_ROWS_WIN_MERGE && out && rows > 0 && C > 0 && C % 8 == 0 &&
               ldo % 8 == 0 && ldo >= C);
  VD_CHECK_ARG(al16(out));
  if (x) VD_CHECK_ARG(al16(x) && ldx % 8 == 0 && ldx >= C);
  if (win) {
    const int64_t F = y_period, hw = y_div, L = ldy, s = win_s;
    VD_CHECK_ARG(x && out != x && L >= 1 && L <= 32 && s >= 1 && s <= L && F >= L && F <= (1 << 20) && hw >= 1);
    VD_CHECK_ARG(hw * (C / 8) <= 0x3fffffff && rows % (F * hw) == 0);
    if (op == VD_ROWS_WIN_MERGE)  // the L weights: fp32 on the device
      VD_CHECK_ARG(y && ((uintptr_t)y & 3) == 0 && y_f32 == 1);
    else
      VD_CHECK_ARG(y == nullptr && y_f32 == 0);
    const int64_t B = rows / (F * hw), nReg = (F - L) / s + 1, nW = nReg + ((nReg - 1) * s + L < F ? 1 : 0);
    const int64_t gx = op == VD_ROWS_WIN_GATHER ? B * nW * L : B * F;
    VD_CHECK_ARG(gx <= 0x7fffffff);
    const int64_t cpr = C / 8, by = (hw * cpr + NT - 1) / NT, gy = by < 4096 ? by : 4096;
    const WinGeo g{(int)F, (int)L, (int)s, (int)nReg, (int)nW, (int)hw, (int)cpr, (int)(gy * NT / cpr),
                   (int)(gy * NT % cpr)};
    if (op == VD_ROWS_WIN_GATHER)
      hipLaunchKernelGGL(win_gather_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(NT), 0, (hipStream_t)stream,
                         (const bf16_t*)x, ldx, g, (bf16_t*)out, ldo);
    else
      hipLaunchKernelGGL(win_merge_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(NT), 0, (hipStream_t)stream,
                         (const bf16_t*)x, ldx, (const float*)y, g, (bf16_t*)out, ldo);
    return vd_launch_status();
  }
  if (op == 0) {
    VD_CHECK_ARG(y && al16(y) && ldy >= C && ldy % (y_f32 ? 4 : 8) == 0 && y_div > 0 && y_period > 0);
  } else {
    VD_CHECK_ARG(x != nullptr);
  }
  if (op == VD_ROWS_FREEU_FILTER || op == VD_ROWS_SCALE)  // the scalar: one fp32 on the device
    VD_CHECK_ARG(y && ((uintptr_t)y & 3) == 0 && y_f32 == 1 && ldy == 0);
  if (op == VD_ROWS_FREEU_FILTER) {
    const int64_t H = y_period, W = y_div;
    VD_CHECK_ARG(H >= 2 && W >= 2 && H + W <= 4096 && rows % (H * W) == 0 && out != x);
    const int64_t n_img = rows / (H * W), nchunk = C / 8;
    // the widest slab (one 128-byte line per pixel row at n8 = 8) that still gives every CU two
    // workgroups; a grid that cannot reach that runs one chunk per workgroup
    int n8 = 1;
    for (int w : {8, 4, 2})
      if (nchunk % w == 0 && n_img * (nchunk / w) >= 2 * 256) {
        n8 = w;
        break;
      }
    const int64_t nslab = nchunk / n8, grid = n_img * nslab;
    VD_CHECK_ARG(grid <= 0x7fffffff);
    const unsigned nt = n8 == 1 ? 64 : n8 * FU_L;
    const size_t lds = (FU_RED + 2 * (size_t)(H + W)) * sizeof(float);
    auto kern = H * W <= FU_L * FU_KEEP ? freeu_filter_kernel<true> : freeu_filter_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(nt), lds, (hipStream_t)stream, (const bf16_t*)x, ldx,
                       (const float*)y, (int)H, (int)W, n8, (int)nslab, (bf16_t*)out, ldo);
    return vd_launch_status();
  }
  hipLaunchKernelGGL(rows_eltwise_kernel, dim3(grid_for(rows * (C / 8))), dim3(NT), 0, (hipStream_t)stream, op,
                     (const bf16_t*)x, ldx, y, ldy, y_f32, y_div, y_period, rows, C, (bf16_t*)out, ldo);
  return vd_launch_status();
}

extern "C" int vd_upsample_nearest2x(const void* x, int64_t ldx, int64_t n_img, int64_t h, int64_t w, int64_t C,
                                     void* out, int64_t ldo, vd_stream_t stream) {
  VD_CHECK_ARG(x && out && al16(x) && al16(out) && n_img > 0 && h > 0 && w > 0 && C > 0 && C % 8 == 0);
  VD_CHECK_ARG(ldx % 8 == 0 && ldo % 8 == 0 && ldx >= C && ldo >= C);
  hipLaunchKernelGGL(upsample2x_kernel, dim3(grid_for(n_img * 4 * h * w * (C / 8))), dim3(NT), 0, (hipStream_t)stream,
                     (const bf16_t*)x, ldx, n_img, h, w, C, (bf16_t*)out, ldo);
  return vd_launch_status();
}
