// What the GEMM files share (gemm.hip: plan, checks, dispatch; gemm_v1 / v2 / v3 / v5 / v6 / v8.hip:
// one kernel family and its launch each; gemm_splitk.hip: the split-K reduce).
//  * device helpers used by more than one family, in an anonymous namespace (each file
//    compiles its own copy; they are all force-inlined);
//  * the tile constants of every family that the plan reads;
//  * the Plan, and the host functions that cross files, in one namespace with hidden
//    visibility: nothing here is part of the library's ABI (include/vdiff.h).
// There is no relocatable device code: a kernel lives in the file of the launch that starts it.
//
// Orientation (every family): the MFMA computes C^T = W . A^T, i.e. the weight tile is the
// MFMA A operand (rows = output channels n) and the activation tile the B
// operand (rows = pixels/tokens m).  With v_mfma_f32_16x16x32_bf16 each lane
// then owns 4 CONSECUTIVE output channels of one pixel, so the NHWC store is
// one 8-byte (bf16) / 16-byte (fp32) write per lane and the GEGLU pair
// (hidden block, gate block) lands in the same lane.
#pragma once
#include "common.h"

namespace {

constexpr int BK = 64;    // K elements per LDS tile row (128 bytes = 8 chunks)
constexpr int NT = 256;   // threads per block (v1)

// A byte offset no buffer resource of these kernels reaches (every operand is checked to be
// smaller): a buffer load from it returns zero, a buffer store to it is dropped.
constexpr uint32_t G2_OOB = 0x80000000u;

// tile constants by family (the kernels' comment blocks are in their files)
constexpr int G9_NW = 4, G9_U = 8, G9_MMAX = 16;
constexpr int G2_BM = 256, G2_NT = 512, G2_STAGES = 3;
constexpr int G3_BM = 256, G3_BN = 256, G3_NT = 512;
constexpr int G4_BM = 256, G4_BK = 32;
constexpr int G6_BM = 64, G6_BN = 64, G6_NT = 256;
constexpr int G8_BN = 160, G8_KMAX = 320, G8_NW = 8;

// The conv kernels' MODE template argument is vd_gemm_desc.a_mode, or A_CONV_PAD_END for a
// VD_A_CONV3X3 descriptor that came with stride 2 | VD_CONV_PAD_END (vd_gemm strips the flag, so
// the kernels see d.stride == 2): instances of their own, so the pad-1 instances are unchanged.
// A tap's input row is oh * stride + dy - conv_pad_lo (column alike); past the far edge the
// loaders' range checks zero it in both modes.
constexpr int A_CONV_PAD_END = 2;
static_assert(A_CONV_PAD_END != VD_A_DENSE && A_CONV_PAD_END != VD_A_CONV3X3, "internal mode");
template <int MODE>
constexpr int conv_pad_lo = MODE == A_CONV_PAD_END ? 0 : 1;
constexpr bool mode_is_conv(int mode) { return mode == VD_A_CONV3X3 || mode == A_CONV_PAD_END; }

__device__ __forceinline__ int lds_off(int row, int chunk) {
  return row * BK + ((chunk ^ (row & 7)) << 3);
}

// a / b for 0 <= a < 2^31 and a wave-uniform b > 0 (round 3): every image size, row width and
// frame count of the UNet is a power of two, so the common case is a shift; hipcc's 32-bit
// division is ~25 VALU, the 64-bit one (an int64 row index) ~100
struct Div {
  int b, sh;
  __device__ __forceinline__ explicit Div(int b_) : b(b_), sh((b_ & (b_ - 1)) == 0 ? __builtin_ctz((uint32_t)b_) : -1) {}
  __device__ __forceinline__ int operator()(int a) const {
    return sh >= 0 ? (int)((uint32_t)a >> sh) : (int)((uint32_t)a / (uint32_t)b);
  }
};

// PERM: the vd_gemm_desc.rmap_* output-row map (instantiated only by the kernels the plan gives
// an rmap request — v6, v1; the v2 / v3 / v5 pipelines sit at 256 VGPRs and spill with it)
template <int MB, int NB, bool PERM = false>
__device__ __forceinline__ void gemm_epilogue(const vd_gemm_desc& d, f32x4 (&acc)[NB][MB], int mbase,
                                              int nbase, int lane, int nodd = -1) {
  // acc[a][b][j] = C[m = mbase + b*16 + fr][n = nbase + a*16 + 4*fq + j]  (the wave's sub-tile);
  // nodd >= 0 moves the odd last block (NB odd) to columns nodd .. nodd + 15 instead
  // All offsets fit 32 bits (M*ldc < 2^31 is checked on the host).
  const int M = (int)d.M, N = (int)d.N;
  const int fr = lane & 15, fq = lane >> 4;
  const int nw = nbase;
  const Rev3 perm = PERM ? Rev3(d.M, d.rmap_n1, d.rmap_n2, d.rmap_inner) : Rev3(0, 0, 0, 0);
  // per-row values are recomputed inside each loop (arrays of MB row pointers kept
  // live across the whole epilogue cost 3 x MB VGPRs beside MB x NB x 4 accumulators)
#define VD_EPI_ROW(b)                                       \
  const int m_ = mbase + (b) * 16 + fr;                     \
  const bool mok_ = m_ < M;                                 \
  const int mrow_ = mok_ ? (PERM ? perm(m_) : m_) : 0;
  // Wide path (T21 for the 16x16 layout): v_permlane16_swap of 16-column blocks
  // (a, a+1) leaves each lane 8 CONSECUTIVE channels — lane group g of the pair
  // holds columns 16a + 16(g&1) + 8(g>>1) .. +7 — so residual loads and bf16
  // stores are 16 B and each store instruction writes 64 contiguous bytes per row
  // (full 64-B write granules) instead of 32.
  const bool wide = (N % 8) == 0 && !d.out_f32 && (d.ldc % 8) == 0 && (((uintptr_t)d.out) & 15) == 0 &&
                    (!d.res || ((d.ld_res % 8) == 0 && (((uintptr_t)d.res) & 15) == 0));
  const int wcol = 16 * (fq & 1) + 8 * (fq >> 1);  // lane's column offset inside a swapped pair
  // the row-bias row of each of the lane's MB rows, divided once (not per column block)
  int rbr[MB];
  if (d.rowbias) {
    const Div rdiv((int)d.rb_div);
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      const int m = mbase + b * 16 + fr;
      rbr[b] = rdiv(m < M ? m : 0);
    }
  }
  if (d.act == VD_ACT_GEGLU) {
    if constexpr (NB % 4 == 0) {
      if (wide) {
        bf16_t* out = (bf16_t*)d.out;
#pragma unroll
        for (int a = 0; a < NB; a += 4) {  // hidden/gate blocks (a, a+1) and (a+2, a+3)
          const int nh0 = nw + a * 16 + 4 * fq, nh1 = nh0 + 32;
          float bh0[4] = {0, 0, 0, 0}, bg0[4] = {0, 0, 0, 0}, bh1[4] = {0, 0, 0, 0}, bg1[4] = {0, 0, 0, 0};
          if (d.bias) {
            const float4 t0 = *(const float4*)(d.bias + (nh0 < N ? nh0 : 0));
            const float4 t1 = *(const float4*)(d.bias + (nh0 + 16 < N ? nh0 + 16 : 0));
            const float4 t2 = *(const float4*)(d.bias + (nh1 < N ? nh1 : 0));
            const float4 t3 = *(const float4*)(d.bias + (nh1 + 16 < N ? nh1 + 16 : 0));
            bh0[0] = t0.x; bh0[1] = t0.y; bh0[2] = t0.z; bh0[3] = t0.w;
            bg0[0] = t1.x; bg0[1] = t1.y; bg0[2] = t1.z; bg0[3] = t1.w;
            bh1[0] = t2.x; bh1[1] = t2.y; bh1[2] = t2.z; bh1[3] = t2.w;
            bg1[0] = t3.x; bg1[1] = t3.y; bg1[2] = t3.z; bg1[3] = t3.w;
          }
          const int nout = nw / 2 + (a / 2) * 16 + wcol;
#pragma unroll
          for (int b = 0; b < MB; ++b) {
            VD_EPI_ROW(b)
            uint32_t x[2], y[2];
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
              const f32x2 go = gelu_erf2(f32x2{acc[a + 1][b][2 * h2], acc[a + 1][b][2 * h2 + 1]} +
                                         f32x2{bg0[2 * h2], bg0[2 * h2 + 1]});
              const f32x2 gp = gelu_erf2(f32x2{acc[a + 3][b][2 * h2], acc[a + 3][b][2 * h2 + 1]} +
                                         f32x2{bg1[2 * h2], bg1[2 * h2 + 1]});
              const f32x2 oo =
                  (f32x2{acc[a][b][2 * h2], acc[a][b][2 * h2 + 1]} + f32x2{bh0[2 * h2], bh0[2 * h2 + 1]}) * go;
              const f32x2 pp =
                  (f32x2{acc[a + 2][b][2 * h2], acc[a + 2][b][2 * h2 + 1]} + f32x2{bh1[2 * h2], bh1[2 * h2 + 1]}) * gp;
              const float o0 = oo[0], o1 = oo[1], p0 = pp[0], p1 = pp[1];
              auto r = __builtin_amdgcn_permlane16_swap(pack2(o0, o1), pack2(p0, p1), false, false);
              x[h2] = r[0];
              y[h2] = r[1];
            }
            if (mok_ && 2 * nout < N)
              *(uint4*)(out + (uint32_t)(mrow_ * (int)d.ldc + nout)) = make_uint4(x[0], x[1], y[0], y[1]);
          }
        }
        return;
      }
    }
    if constexpr (NB % 2 == 0) {
      bf16_t* out = (bf16_t*)d.out;
#pragma unroll
      for (int a = 0; a < NB; a += 2) {
        const int nh = nw + a * 16 + 4 * fq;  // packed hidden column
        const int ng = nh + 16;                // packed gate column
        if (ng >= N) continue;
        const int nout = nw / 2 + (a / 2) * 16 + 4 * fq;
        float bh[4] = {0, 0, 0, 0}, bg[4] = {0, 0, 0, 0};
        if (d.bias) {
          const float4 t0 = *(const float4*)(d.bias + nh);
          const float4 t1 = *(const float4*)(d.bias + ng);
          bh[0] = t0.x; bh[1] = t0.y; bh[2] = t0.z; bh[3] = t0.w;
          bg[0] = t1.x; bg[1] = t1.y; bg[2] = t1.z; bg[3] = t1.w;
        }
#pragma unroll
        for (int b = 0; b < MB; ++b) {
          VD_EPI_ROW(b)
          if (!mok_) continue;
          float o[4];
          const f32x2 g01 = gelu_erf2(f32x2{acc[a + 1][b][0] + bg[0], acc[a + 1][b][1] + bg[1]});
          const f32x2 g23 = gelu_erf2(f32x2{acc[a + 1][b][2] + bg[2], acc[a + 1][b][3] + bg[3]});
          o[0] = (acc[a][b][0] + bh[0]) * g01[0];
          o[1] = (acc[a][b][1] + bh[1]) * g01[1];
          o[2] = (acc[a][b][2] + bh[2]) * g23[0];
          o[3] = (acc[a][b][3] + bh[3]) * g23[1];
          *(uint2*)(out + (uint32_t)(mrow_ * (int)d.ldc + nout)) = make_uint2(pack2(o[0], o[1]), pack2(o[2], o[3]));
        }
      }
    }
    return;
  }
  if (wide) {
    bf16_t* out = (bf16_t*)d.out;
#pragma unroll
    for (int a = 0; a + 1 < NB; a += 2) {
      const int n = nw + a * 16 + wcol;  // first of this lane's 8 columns after the swap
      const bool nok = n < N;
      const int nn = nok ? n : 0;
      float bv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (d.bias) {
        const float4 t0 = *(const float4*)(d.bias + nn), t1 = *(const float4*)(d.bias + nn + 4);
        bv[0] = t0.x; bv[1] = t0.y; bv[2] = t0.z; bv[3] = t0.w;
        bv[4] = t1.x; bv[5] = t1.y; bv[6] = t1.z; bv[7] = t1.w;
      }
      uint4 rsv[MB];  // residual rows loaded together ahead of the stores (as epi_ln, round 2)
      if (d.res) {
#pragma unroll
        for (int b = 0; b < MB; ++b) {
          VD_EPI_ROW(b)
          rsv[b] = *(const uint4*)((const bf16_t*)d.res + (uint32_t)(mrow_ * (int)d.ld_res + nn));
        }
      }
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        VD_EPI_ROW(b)
        float o[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[a][b][j]), __float_as_uint(acc[a + 1][b][j]),
                                                    false, false);
          o[j] = __uint_as_float(r[0]) + bv[j];
          o[4 + j] = __uint_as_float(r[1]) + bv[4 + j];
        }
        if (!mok_ || !nok) continue;
        if (d.rowbias) {
          const float* rbrow = d.rowbias + (int64_t)rbr[b] * d.ld_rb;
          const float4 t0 = *(const float4*)(rbrow + n), t1 = *(const float4*)(rbrow + n + 4);
          o[0] += t0.x; o[1] += t0.y; o[2] += t0.z; o[3] += t0.w;
          o[4] += t1.x; o[5] += t1.y; o[6] += t1.z; o[7] += t1.w;
        }
        if (act_is_pw(d.act)) {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = act_pw(d.act, o[j]);
        }
        if (d.res) {
          float rf[8];
          unpack8(rsv[b], rf);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += rf[j];
        }
        *(uint4*)(out + (uint32_t)(mrow_ * (int)d.ldc + n)) = pack8(o);
      }
    }
    if constexpr (NB % 2 == 0) return;
  }
#pragma unroll
  for (int a = 0; a < NB; ++a) {  // narrow path (or, when wide, the odd last block)
    if (wide && a + 1 < NB) continue;
    const int n = (nodd >= 0 && a == NB - 1 ? nodd : nw + a * 16) + 4 * fq;
    if (n >= N) continue;
    float bv[4] = {0, 0, 0, 0};
    if (d.bias) {
      const float4 t = *(const float4*)(d.bias + n);
      bv[0] = t.x; bv[1] = t.y; bv[2] = t.z; bv[3] = t.w;
    }
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      VD_EPI_ROW(b)
      if (!mok_) continue;
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = acc[a][b][j] + bv[j];
      if (d.rowbias) {
        const float4 t = *(const float4*)(d.rowbias + (int64_t)rbr[b] * d.ld_rb + n);
        o[0] += t.x; o[1] += t.y; o[2] += t.z; o[3] += t.w;
      }
      if (act_is_pw(d.act)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = act_pw(d.act, o[j]);
      }
      if (d.res) {
        const uint2 r = *(const uint2*)((const bf16_t*)d.res + (uint32_t)(mrow_ * (int)d.ld_res + n));
        o[0] += bf_lo(r.x); o[1] += bf_hi(r.x); o[2] += bf_lo(r.y); o[3] += bf_hi(r.y);
      }
      const uint32_t off = (uint32_t)(mrow_ * (int)d.ldc + n);
      if (d.out_f32) {
        *(float4*)((float*)d.out + off) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
        *(uint2*)((bf16_t*)d.out + off) = make_uint2(pack2(o[0], o[1]), pack2(o[2], o[3]));
      }
    }
  }
}

#undef VD_EPI_ROW

typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* lds, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)lds, 16, voff, 0, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  else static_assert(N == 0, "unsupported vmcnt");
}

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// Load-free epilogue (v5, split == 1, bf16 out, no residual / row bias): the bias
// comes from the unit's LDS slot (DMA'd with its first k-step) and every store is
// an UNCONDITIONAL buffer store whose out-of-range lanes carry an offset past the
// resource's num_records (dropped by the hardware).  So the epilogue issues no
// vector-memory load — nothing makes the wave wait for the k-steps still in flight
// — and a compile-time number of stores, which the k-loop's counted vmcnt then
// leaves outstanding instead of draining.  Returns that number.
template <int MB, int NB>
__device__ __forceinline__ int epi_fast(const vd_gemm_desc& d, f32x4 (&acc)[NB][MB], int mbase, int nbase, int lane,
                                        const float* bsl, int n0, __amdgpu_buffer_rsrc_t ro) {
  static_assert(NB % 2 == 0, "epi_fast: whole 16-column pairs");
  const int M = (int)d.M, N = (int)d.N, ldc = (int)d.ldc;
  const int fr = lane & 15, fq = lane >> 4;
  const int wcol = 16 * (fq & 1) + 8 * (fq >> 1);
  int nst = 0;
  if (d.act == VD_ACT_GEGLU) {
    // pairs (a, a+1) = (hidden, gate) blocks -> 16 output columns; pair-pairs swapped
    // by permlane16 into 8 consecutive columns per lane (16-B stores), a lone last
    // pair stores 4 columns (8 B)
    constexpr int NP = NB / 2;
#pragma unroll
    for (int pp = 0; pp + 1 < NP; pp += 2) {
      const int a = 2 * pp;
      const int c0 = nbase - n0 + a * 16 + 4 * fq;  // column of acc[a][.][0] inside the tile
      const float4 th0 = *(const float4*)(bsl + c0), tg0 = *(const float4*)(bsl + c0 + 16);
      const float4 th1 = *(const float4*)(bsl + c0 + 32), tg1 = *(const float4*)(bsl + c0 + 48);
      const float bh0[4] = {th0.x, th0.y, th0.z, th0.w}, bg0[4] = {tg0.x, tg0.y, tg0.z, tg0.w};
      const float bh1[4] = {th1.x, th1.y, th1.z, th1.w}, bg1[4] = {tg1.x, tg1.y, tg1.z, tg1.w};
      const int nout = nbase / 2 + pp * 16 + wcol;
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        const int m = mbase + b * 16 + fr;
        uint32_t x[2], y[2];
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          // (h + bh) * gelu(g + bg) on value pairs: packed adds / multiplies, the same bits
          const f32x2 go = gelu_erf2(f32x2{acc[a + 1][b][2 * h2], acc[a + 1][b][2 * h2 + 1]} +
                                     f32x2{bg0[2 * h2], bg0[2 * h2 + 1]});
          const f32x2 gp = gelu_erf2(f32x2{acc[a + 3][b][2 * h2], acc[a + 3][b][2 * h2 + 1]} +
                                     f32x2{bg1[2 * h2], bg1[2 * h2 + 1]});
          const f32x2 oo = (f32x2{acc[a][b][2 * h2], acc[a][b][2 * h2 + 1]} + f32x2{bh0[2 * h2], bh0[2 * h2 + 1]}) * go;
          const f32x2 pp = (f32x2{acc[a + 2][b][2 * h2], acc[a + 2][b][2 * h2 + 1]} + f32x2{bh1[2 * h2], bh1[2 * h2 + 1]}) * gp;
          const float o0 = oo[0], o1 = oo[1], p0 = pp[0], p1 = pp[1];
          auto r = __builtin_amdgcn_permlane16_swap(pack2(o0, o1), pack2(p0, p1), false, false);
          x[h2] = r[0];
          y[h2] = r[1];
        }
        const bool ok = m < M && 2 * nout < N;
        const uint32_t off = ok ? (uint32_t)(m * ldc + nout) * 2u : G2_OOB;
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{x[0], x[1], y[0], y[1]}, ro, off, 0, 0);
        ++nst;
      }
    }
    if constexpr (NP % 2 == 1) {
      const int a = NB - 2;
      const int c0 = nbase - n0 + a * 16 + 4 * fq;
      const float4 th = *(const float4*)(bsl + c0), tg = *(const float4*)(bsl + c0 + 16);
      const float bh[4] = {th.x, th.y, th.z, th.w}, bg[4] = {tg.x, tg.y, tg.z, tg.w};
      const int nout = nbase / 2 + (a / 2) * 16 + 4 * fq;
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        const int m = mbase + b * 16 + fr;
        float o[4];
        const f32x2 g01 = gelu_erf2(f32x2{acc[a + 1][b][0] + bg[0], acc[a + 1][b][1] + bg[1]});
        const f32x2 g23 = gelu_erf2(f32x2{acc[a + 1][b][2] + bg[2], acc[a + 1][b][3] + bg[3]});
        o[0] = (acc[a][b][0] + bh[0]) * g01[0];
        o[1] = (acc[a][b][1] + bh[1]) * g01[1];
        o[2] = (acc[a][b][2] + bh[2]) * g23[0];
        o[3] = (acc[a][b][3] + bh[3]) * g23[1];
        const bool ok = m < M && 2 * nout < N;
        const uint32_t off = ok ? (uint32_t)(m * ldc + nout) * 2u : G2_OOB;
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{pack2(o[0], o[1]), pack2(o[2], o[3])}, ro, off, 0, 0);
        ++nst;
      }
    }
    return nst;
  }
#pragma unroll
  for (int a = 0; a < NB; a += 2) {
    const int n = nbase + a * 16 + wcol;  // first of this lane's 8 columns after the swap
    const float4 t0 = *(const float4*)(bsl + (n - n0)), t1 = *(const float4*)(bsl + (n - n0) + 4);
    const float bv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      const int m = mbase + b * 16 + fr;
      float o[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[a][b][j]), __float_as_uint(acc[a + 1][b][j]),
                                                  false, false);
        o[j] = __uint_as_float(r[0]) + bv[j];
        o[4 + j] = __uint_as_float(r[1]) + bv[4 + j];
      }
      if (act_is_pw(d.act)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = act_pw(d.act, o[j]);
      }
      const uint4 pk = pack8(o);
      const bool ok = m < M && n < N;
      const uint32_t off = ok ? (uint32_t)(m * ldc + n) * 2u : G2_OOB;
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{pk.x, pk.y, pk.z, pk.w}, ro, off, 0, 0);
      ++nst;
    }
  }
  return nst;
}

// s_waitcnt vmcnt(n) (expcnt / lgkmcnt left at max) for a wave-uniform runtime n;
// n > 63 waits for 63 (more than asked: always safe).
template <int N>
__device__ __forceinline__ void s_wait_vm() {
  __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4) | (0xF << 8));
}
__device__ __forceinline__ void wait_vm_rt(int n) {
#define VM4(B) case B: s_wait_vm<B>(); break; case B + 1: s_wait_vm<B + 1>(); break; \
               case B + 2: s_wait_vm<B + 2>(); break; case B + 3: s_wait_vm<B + 3>(); break;
  switch (n) {
    VM4(0) VM4(4) VM4(8) VM4(12) VM4(16) VM4(20) VM4(24) VM4(28)
    VM4(32) VM4(36) VM4(40) VM4(44) VM4(48) VM4(52) VM4(56) VM4(60)
    default: s_wait_vm<63>(); break;
  }
#undef VM4
}

}  // namespace

namespace vdgemm __attribute__((visibility("hidden"))) {

// What the plan (gemm.hip) hands a launch: the kernel family, its N tile, the K split, and the
// operands' sizes in bytes for the buffer descriptors of the LDS-DMA kernels (0 on v1 / v9).
struct Plan {
  int ver = 1;
  int bn = 128, split = 1;
  bool ln_fused = false;  // v5 writes ln_out in its epilogue
  bool pad_end = false;   // the A_CONV_PAD_END instance; set by vd_gemm, not by the plan
  uint32_t a0b = 0, a1b = 0, wb = 0;
  int64_t ws_bytes = 0;
};

// the device's CU count, read once per process (256, the MI355X's, without a device): the plan,
// the workspace size and the persistent grids depend on it
int num_cus();

// persistent kernels (v2, v3, v5): one workgroup per CU, ceil(units / CUs) rounds, balanced grid
inline int64_t persistent_grid(int64_t units) {
  const int64_t rounds = (units + num_cus() - 1) / num_cus();
  return (units + rounds - 1) / rounds;
}

int launch_v1(const vd_gemm_desc& d, const Plan& p, hipStream_t s);  // p.bn: 128 x {64, 128, 160}
int launch_v9(const vd_gemm_desc& d, hipStream_t s);
int launch_v2(const vd_gemm_desc& d, const Plan& p, hipStream_t s);  // p.bn: 256 x {32, 128, 160}
int launch_v3(const vd_gemm_desc& d, const Plan& p, hipStream_t s);
int launch_v5(const vd_gemm_desc& d, const Plan& p, hipStream_t s);
int launch_v6(const vd_gemm_desc& d, const Plan& p, hipStream_t s);
int launch_v8(const vd_gemm_desc& d, const Plan& p, hipStream_t s);
// sums the split fp32 slabs of d.ws and applies the epilogue (after a split v2 / v3 / v5 launch)
int launch_splitk_reduce(const vd_gemm_desc& d, int split, hipStream_t s);

}  // namespace vdgemm
