// vd_rows_eltwise op 6, FreeInit's 3-D spectral low-pass (diffusers' free_init_utils
// _apply_freq_filter) over fp32 volumes of F x H x W points, as five axis passes
// (include/vdiff.h has the call geometry):
//   out = y + Re(IDFT3(M * DFT3(x - y))),   M the caller's Hermitian-even table in DFT order,
// so only the half spectrum kw <= W / 2 is ever held: real-to-complex along W, complex along H,
// then along F, the table, and the same three back.  The complex half spectrum lives in the
// caller's scratch; the library allocates nothing.
//
// Every pass is a direct O(N^2) DFT out of LDS.  A workgroup loads whole lines (a chunk of
// neighbouring lines, so that a row's bytes are contiguous over adjacent threads), then one
// thread forms one output point from the line in LDS, which is what lets passes 2 to 4 run in
// place.  The twiddles are a per-workgroup LDS table of N entries, cos / sin(2 pi j / N) from
// double-precision sincospi rounded once to fp32, indexed by (n k) mod N kept in integers.
// A point is the sum of four interleaved partial sums (n mod 4, fmaf per term, ascending n),
// combined as (s0 + s1) + (s2 + s3): the order depends on N alone, never on the chunking, the
// number of volumes, a volume's index or the row strides, so results are bitwise reproducible
// across all of them.  No atomics.
#include "common.h"

namespace {

constexpr int SP_NT = 256;
constexpr int SP_TILE = 2048;  // complex points of one LDS tile (16 KiB)

__device__ __forceinline__ void sp_fill_twiddles(float2* tw, int N) {
  for (int j = threadIdx.x; j < N; j += SP_NT) {
    double sn, cs;
    sincospi(2.0 * (double)j / (double)N, &sn, &cs);  // the argument is in [0, 2): nothing to reduce
    tw[j] = make_float2((float)cs, (float)sn);
  }
}

// sum over n < N of v[n * vs] * exp(SIGN * 2 pi i n k / N)
template <int SIGN>
__device__ __forceinline__ float2 sp_point(const float2* v, int vs, const float2* tw, int N, int k) {
  float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
  int idx = 0;
  for (int n0 = 0; n0 < N; n0 += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (n0 + q < N) {
        const float2 a = v[(n0 + q) * vs], t = tw[idx];
        if (SIGN < 0) {  // (a.x + i a.y)(c - i s)
          re[q] = fmaf(a.x, t.x, re[q]);
          re[q] = fmaf(a.y, t.y, re[q]);
          im[q] = fmaf(a.y, t.x, im[q]);
          im[q] = fmaf(-a.x, t.y, im[q]);
        } else {  // (a.x + i a.y)(c + i s)
          re[q] = fmaf(a.x, t.x, re[q]);
          re[q] = fmaf(-a.y, t.y, re[q]);
          im[q] = fmaf(a.y, t.x, im[q]);
          im[q] = fmaf(a.x, t.y, im[q]);
        }
        idx += k;
        if (idx >= N) idx -= N;
      }
    }
  }
  return make_float2((re[0] + re[1]) + (re[2] + re[3]), (im[0] + im[1]) + (im[2] + im[3]));
}

// pass 1: S[r][kw] = sum_w (x[r][w] - y[r][w]) exp(-2 pi i w kw / W), kw < Wh; R rows a workgroup
__global__ __launch_bounds__(SP_NT) void spectral_r2c_kernel(const float* x, int64_t ldx, const float* y,
                                                             int64_t ldy, int64_t rows, int W, int Wh, int R,
                                                             float* S, int64_t lds) {
  extern __shared__ __attribute__((aligned(16))) float sp_smem[];
  float2* tw = (float2*)sp_smem;  // [W]
  float* d = sp_smem + 2 * W;     // [R][W]
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int nr = (int)(rows - row0 < R ? rows - row0 : R);
  sp_fill_twiddles(tw, W);
  for (int i = threadIdx.x; i < nr * W; i += SP_NT) {
    const int r = i / W, w = i - r * W;
    d[i] = x[(row0 + r) * ldx + w] - y[(row0 + r) * ldy + w];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < nr * Wh; o += SP_NT) {
    const int r = o / Wh, k = o - r * Wh;
    const float* v = d + r * W;
    float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
    int idx = 0;
    for (int n0 = 0; n0 < W; n0 += 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (n0 + q < W) {
          const float a = v[n0 + q];
          const float2 t = tw[idx];
          re[q] = fmaf(a, t.x, re[q]);
          im[q] = fmaf(-a, t.y, im[q]);
          idx += k;
          if (idx >= W) idx -= W;
        }
      }
    }
    *(float2*)(S + (row0 + r) * lds + 2 * k) =
        make_float2((re[0] + re[1]) + (re[2] + re[3]), (im[0] + im[1]) + (im[2] + im[3]));
  }
}

// passes 2 to 4: lines of N points along H (inner = 1) or F (inner = H), in place.  Line group
// g = blockIdx.x / nchunk starts at row (g / inner) * inner * N + g % inner and steps `inner`
// rows; the workgroup holds columns kw0 .. kw0 + ch of it.
//   MODE 0: forward   MODE 1: inverse (unscaled)
//   MODE 2: forward, times table[k][g % inner][kw], inverse (unscaled), the line never leaving LDS
template <int MODE>
__global__ __launch_bounds__(SP_NT) void spectral_line_kernel(float* S, int64_t lds, const float* table, int N,
                                                              int inner, int Wh, int CH, int nchunk) {
  extern __shared__ __attribute__((aligned(16))) float sp_smem[];
  float2* tw = (float2*)sp_smem;  // [N]
  float2* a = tw + N;             // [N][CH]
  float2* b = a + N * CH;         // [N][CH], MODE 2 only
  const int g = blockIdx.x / nchunk, kw0 = (blockIdx.x - g * nchunk) * CH;
  const int ch = Wh - kw0 < CH ? Wh - kw0 : CH;
  const int gi = g % inner;
  const int64_t row0 = (int64_t)(g / inner) * inner * N + gi;
  sp_fill_twiddles(tw, N);
  for (int i = threadIdx.x; i < N * ch; i += SP_NT) {
    const int n = i / ch, c = i - n * ch;
    a[n * CH + c] = *(const float2*)(S + (row0 + (int64_t)n * inner) * lds + 2 * (kw0 + c));
  }
  __syncthreads();
  if (MODE == 2) {
    for (int o = threadIdx.x; o < N * ch; o += SP_NT) {
      const int k = o / ch, c = o - k * ch;
      const float2 f = sp_point<-1>(a + c, CH, tw, N, k);
      const float m = table[((int64_t)k * inner + gi) * Wh + kw0 + c];
      b[k * CH + c] = make_float2(f.x * m, f.y * m);
    }
    __syncthreads();
  }
  const float2* src = MODE == 2 ? b : a;
  for (int o = threadIdx.x; o < N * ch; o += SP_NT) {
    const int k = o / ch, c = o - k * ch;
    const float2 f = MODE == 0 ? sp_point<-1>(src + c, CH, tw, N, k) : sp_point<1>(src + c, CH, tw, N, k);
    *(float2*)(S + (row0 + (int64_t)k * inner) * lds + 2 * (kw0 + c)) = f;
  }
}

// pass 5: out[r][w] = y[r][w] + (sum_kw m_kw Re(S[r][kw] exp(2 pi i kw w / W))) / cnt, m = 1 for
// kw = 0 and for kw = W / 2 of an even W, 2 for the bins whose mirror is not stored
__global__ __launch_bounds__(SP_NT) void spectral_c2r_kernel(const float* S, int64_t lds, const float* y,
                                                             int64_t ldy, int64_t rows, int W, int Wh, int R,
                                                             float cnt, float* out, int64_t ldo) {
  extern __shared__ __attribute__((aligned(16))) float sp_smem[];
  float2* tw = (float2*)sp_smem;  // [W]
  float2* s = tw + W;             // [R][Wh], pre-multiplied by m
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int nr = (int)(rows - row0 < R ? rows - row0 : R);
  sp_fill_twiddles(tw, W);
  for (int i = threadIdx.x; i < nr * Wh; i += SP_NT) {
    const int r = i / Wh, k = i - r * Wh;
    const float2 v = *(const float2*)(S + (row0 + r) * lds + 2 * k);
    const float m = (k == 0 || 2 * k == W) ? 1.0f : 2.0f;  // a power of two: exact
    s[i] = make_float2(v.x * m, v.y * m);
  }
  __syncthreads();
  for (int o = threadIdx.x; o < nr * W; o += SP_NT) {
    const int r = o / W, w = o - r * W;
    const float2* v = s + r * Wh;
    float re[4] = {0.f, 0.f, 0.f, 0.f};
    int idx = 0;
    for (int n0 = 0; n0 < Wh; n0 += 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (n0 + q < Wh) {
          const float2 a = v[n0 + q], t = tw[idx];
          re[q] = fmaf(a.x, t.x, re[q]);
          re[q] = fmaf(-a.y, t.y, re[q]);
          idx += w;
          if (idx >= W) idx -= W;
        }
      }
    }
    const float sum = (re[0] + re[1]) + (re[2] + re[3]);
    out[(row0 + r) * ldo + w] = y[(row0 + r) * ldy + w] + sum / cnt;
  }
}

inline bool sp_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// The launch behind vd_rows_eltwise op 6 (rows.hip forwards every argument but the op's low byte).
namespace vdrows __attribute__((visibility("hidden"))) {
int spectral_launch(int32_t pass, const void* x, int64_t ldx, const void* y, int64_t ldy, int32_t y_f32,
                       int64_t H, int64_t F, int64_t rows, int64_t W, void* out, int64_t ldo, vd_stream_t stream) {
  VD_CHECK_ARG(pass >= 1 && pass <= 5 && x && out && sp_al16(x) && sp_al16(out));
  VD_CHECK_ARG(F >= 1 && F <= VD_SPECTRAL_MAX && H >= 1 && H <= VD_SPECTRAL_MAX && W >= 1 && W <= VD_SPECTRAL_MAX);
  VD_CHECK_ARG(rows > 0 && rows % (F * H) == 0 && rows <= 0x3fffffff);
  const int64_t Wh = W / 2 + 1, ldc = 2 * Wh;  // a complex row in floats
  const hipStream_t st = (hipStream_t)stream;
  if (pass == 1 || pass == 5) {
    // x - y in, or + y out: the noise rows
    VD_CHECK_ARG(out != x && y && sp_al16(y) && y_f32 == 1 && ldy >= W);
    const int64_t lds = pass == 1 ? ldo : ldx;
    VD_CHECK_ARG(lds >= ldc && lds % 2 == 0 && (pass == 1 ? ldx : ldo) >= W);
    const int R = (int)(SP_TILE / (pass == 1 ? W : Wh) < 16 ? SP_TILE / (pass == 1 ? W : Wh) : 16);
    const unsigned grid = (unsigned)((rows + R - 1) / R);
    if (pass == 1) {
      const size_t smem = (2 * (size_t)W + (size_t)R * W) * sizeof(float);
      hipLaunchKernelGGL(spectral_r2c_kernel, dim3(grid), dim3(SP_NT), smem, st, (const float*)x, ldx,
                         (const float*)y, ldy, rows, (int)W, (int)Wh, R, (float*)out, ldo);
    } else {
      const size_t smem = (2 * (size_t)W + 2 * (size_t)R * Wh) * sizeof(float);
      hipLaunchKernelGGL(spectral_c2r_kernel, dim3(grid), dim3(SP_NT), smem, st, (const float*)x, ldx,
                         (const float*)y, ldy, rows, (int)W, (int)Wh, R, (float)(F * H * W), (float*)out, ldo);
    }
    return vd_launch_status();
  }
  // passes 2 to 4: in place on the scratch
  VD_CHECK_ARG(out == x && ldo == ldx && ldx >= ldc && ldx % 2 == 0);
  if (pass == 3)  // the table: [F][H][Wh] fp32, contiguous
    VD_CHECK_ARG(y && sp_al16(y) && y_f32 == 1 && ldy == Wh);
  else
    VD_CHECK_ARG(y == nullptr && y_f32 == 0);
  const int64_t N = pass == 3 ? F : H, inner = pass == 3 ? H : 1;
  int64_t CH = SP_TILE / N < 16 ? SP_TILE / N : 16;
  if (CH > Wh) CH = Wh;
  // even chunks: Wh = 33 runs as 3 x 11 columns, not 16 + 16 + 1
  const int64_t nchunk = (Wh + CH - 1) / CH;
  CH = (Wh + nchunk - 1) / nchunk;
  const int64_t grid = rows / N * nchunk;
  VD_CHECK_ARG(grid <= 0x7fffffff);
  const size_t smem = (size_t)(N + (pass == 3 ? 2 : 1) * N * CH) * sizeof(float2);
  auto kern = pass == 2 ? spectral_line_kernel<0> : pass == 3 ? spectral_line_kernel<2> : spectral_line_kernel<1>;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(SP_NT), smem, st, (float*)out, ldx, (const float*)y, (int)N,
                     (int)inner, (int)Wh, (int)CH, (int)nchunk);
  return vd_launch_status();
}
}  // namespace vdrows
