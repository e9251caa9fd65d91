// temporal_attn_kernel — the motion-module attention over F <= 32 frames
// (a9).  Tiny per item (16x16 scores), so VALU with one wave per (position,
// head) and K/V staged in LDS; tokens are read in place from the NHWC rows.
#include <type_traits>

#include "attention_common.h"

namespace {

// One wave per (b, p, h) item; lane = (query f = lane / LPQ, part = lane % LPQ);
// 16-byte dim chunks c of the head are owned by part c % LPQ.
template <int FMAX>
__global__ __launch_bounds__(NT) void temporal_attn_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    int64_t ld, bf16_t* __restrict__ o, int64_t ldo, int64_t batch, int frames, int64_t positions,
    int heads, int d, float scale_log2) {
  constexpr int LPQ = 64 / FMAX;
  __shared__ __attribute__((aligned(16))) bf16_t kv_lds[4][2][FMAX * 160];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t item = (int64_t)blockIdx.x * 4 + wave;
  const int64_t nitems = batch * positions * heads;
  if (item >= nitems) return;
  const int h = (int)(item % heads);
  const int64_t bp = item / heads;
  const int64_t p = bp % positions, b = bp / positions;
  const int nch = d / 8;
  bf16_t* kl = kv_lds[wave][0];
  bf16_t* vl = kv_lds[wave][1];
  // stage K, V of this item: frames x d
  for (int idx = lane; idx < frames * nch; idx += 64) {
    const int f = idx / nch, c = idx - f * nch;
    const int64_t row = (b * frames + f) * positions + p;
    *(uint4*)(kl + f * d + c * 8) = *(const uint4*)(k + row * ld + (int64_t)h * d + c * 8);
    *(uint4*)(vl + f * d + c * 8) = *(const uint4*)(v + row * ld + (int64_t)h * d + c * 8);
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const int fq = lane / LPQ, part = lane % LPQ;
  const bool qvalid = fq < frames;
  const int64_t qrow = (b * frames + (qvalid ? fq : 0)) * positions + p;
  constexpr int MAXC = (20 + LPQ - 1) / LPQ;  // chunks per lane (d <= 160)
  float qv[MAXC][8];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = part + i * LPQ;
    if (c < nch) unpack8(*(const uint4*)(q + qrow * ld + (int64_t)h * d + c * 8), qv[i]);
  }
  float sc[FMAX];
#pragma unroll
  for (int kk = 0; kk < FMAX; ++kk) {
    float acc = 0.f;
    if (kk < frames) {
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int c = part + i * LPQ;
        if (c < nch) {
          float kf[8];
          unpack8(*(const uint4*)(kl + kk * d + c * 8), kf);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc = fmaf(qv[i][e], kf[e], acc);
        }
      }
    }
#pragma unroll
    for (int off = 1; off < LPQ; off <<= 1) acc += __shfl_xor(acc, off, 64);
    sc[kk] = kk < frames ? acc * scale_log2 : -INFINITY;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int kk = 0; kk < FMAX; ++kk) mx = fmaxf(mx, sc[kk]);
  float sum = 0.f;
#pragma unroll
  for (int kk = 0; kk < FMAX; ++kk) {
    sc[kk] = exp2f(sc[kk] - mx);
    sum += sc[kk];
  }
  const float inv = 1.0f / sum;
  if (!qvalid) return;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = part + i * LPQ;
    if (c < nch) {
      float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int kk = 0; kk < FMAX; ++kk) {
        if (kk < frames) {
          float vf[8];
          unpack8(*(const uint4*)(vl + kk * d + c * 8), vf);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] = fmaf(sc[kk], vf[e], acc[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] *= inv;
      *(uint4*)(o + qrow * ldo + (int64_t)h * d + c * 8) = pack8(acc);
    }
  }
}

// ------------------------------------------------------- temporal (MFMA)
// frames <= 16: one (b, p, h) item per wave iteration on v_mfma_f32_16x16x32_bf16.
//   S^T[key][q] = K . Q^T   A = K rows, B = Q^T, both straight from the NHWC rows
//                           (lane (fr, fq) holds row fr, dims 32*ks + 8*fq .. +7);
//   softmax over the 16 keys of query fr: 4 keys per lane, two xor-shuffles;
//   O^T[d][q] = V^T . P^T   P^T's k-slot (fq, j) is key 4*fq + j for j < 4 and an
//                           empty slot (P = 0) for j >= 4, so the S^T accumulator
//                           IS the B operand (no lane movement); V^T comes from a
//                           per-wave LDS image with ds_read_b64_tr_b16 (T10), whose
//                           column D is 1.0: row D of O^T is the softmax row sum.
// Memory-bound (3 reads + 1 write of the head's 16 rows); 4 waves per block,
// items strided over the grid so the LDS padding is written once per wave.
template <int D>
struct TmCfg {
  static constexpr int KSTEPS = (D + 31) / 32;
  static constexpr int DB = (D + 1 + 15) / 16;   // O^T row blocks incl. the ones row
  static constexpr int VS = 16 * (DB | 1);       // LDS row (elements): 32 B x odd -> conflict-free tr reads
  static constexpr int DCH = D / 8;
};

// Query and key frames may differ (vd_temporal_attention_kv: a frame-sharded rank's own
// qframes queries against all kframes keys gathered from every rank, SURVEY §8e's K/V
// all-gather); q/o rows are (b, qframes, p) at stride ldq/ldo, k/v rows (b, kframes, p) at
// stride ldkv.  The self-attention call passes qframes == kframes and one stride.
template <int D>
__global__ __launch_bounds__(NT) void temporal_mfma_kernel(
    const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    int64_t ldkv, bf16_t* __restrict__ o, int64_t ldo, int64_t batch, int qframes, int frames, int64_t positions,
    int heads, float c) {
  using C = TmCfg<D>;
  __shared__ __attribute__((aligned(16))) bf16_t vimg[4][16 * C::VS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  bf16_t* vl = vimg[wave];
  // padding columns [D, VS) of every row: 1.0 at column D, 0 elsewhere (never overwritten);
  // rows >= frames stay zero (their P is 0)
  for (int idx = lane; idx < 16 * C::VS / 8; idx += 64) *(uint4*)(vl + idx * 8) = make_uint4(0, 0, 0, 0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane < 16) vl[lane * C::VS + D] = (bf16_t)0x3F80;
  const int64_t nitems = batch * positions * heads;
  const int64_t stride = (int64_t)gridDim.x * 4;
  const bool unitc = c == 1.0f;
  const int vtr = (4 * fq + (fr >> 2)) * C::VS + 4 * (fr & 3);  // tr-read lane offset in a column block
  // XCD-aware (T1): the blocks holding the other heads of the same position (whose 80-byte
  // head slices share 128-byte lines of the Q/K/V/O rows) get adjacent logical ids, which
  // xcd_remap keeps on one XCD, so a shared line is fetched into one L2, not two
  const int64_t lblk = xcd_remap(blockIdx.x, gridDim.x);
  // Software-pipelined (round 2): the K/Q fragments and V chunks of the wave's NEXT item are
  // loaded into registers while the current item computes, so a wave keeps one item of loads
  // in flight behind its MFMAs, softmax and stores (the kernel is memory-latency bound: 3.3
  // TB/s at L1 with one item's loads outstanding at a time).
  constexpr int VN = (16 * C::DCH + 63) / 64;  // V chunks per lane (frames <= 16)
  const bool fok = fr < frames, qok = fr < qframes;
  uint4 kn[C::KSTEPS], qn[C::KSTEPS], vn[VN];
  // (a macro, not a lambda: a lambda capturing the register arrays by reference left them on
  // the scratch stack)
#define TM_LOAD_ITEM(IT)                                                                              \
  {                                                                                                   \
    const int h_ = (int)((IT) % heads);                                                              \
    const int64_t bp_ = (IT) / heads;                                                                 \
    const int64_t p_ = bp_ % positions, b_ = bp_ / positions;                                         \
    const int64_t row0_ = b_ * frames * positions + p_;                                               \
    const int64_t rf_ = (row0_ + (fok ? fr : 0) * positions) * ldkv + (int64_t)h_ * D;                \
    const int64_t rq_ = ((b_ * qframes * positions + p_) + (qok ? fr : 0) * positions) * ldq + (int64_t)h_ * D; \
    _Pragma("unroll") for (int ks = 0; ks < C::KSTEPS; ++ks) {                                        \
      const int dd = ks * 32 + 8 * fq;                                                                \
      kn[ks] = make_uint4(0, 0, 0, 0);                                                                \
      qn[ks] = make_uint4(0, 0, 0, 0);                                                                \
      if (dd < D) {                                                                                   \
        if (fok) kn[ks] = *(const uint4*)(k + rf_ + dd);                                              \
        if (qok) qn[ks] = *(const uint4*)(q + rq_ + dd);                                              \
      }                                                                                               \
    }                                                                                                 \
    _Pragma("unroll") for (int r = 0; r < VN; ++r) {                                                  \
      const int idx = lane + 64 * r;                                                                  \
      const int f = idx / C::DCH, cc = idx - f * C::DCH;                                              \
      vn[r] = make_uint4(0, 0, 0, 0);                                                                 \
      if (idx < frames * C::DCH)                                                                      \
        vn[r] = *(const uint4*)(v + (row0_ + (int64_t)f * positions) * ldkv + (int64_t)h_ * D + cc * 8); \
    }                                                                                                 \
  }
  int64_t item = lblk * 4 + wave;
  if (item < nitems) TM_LOAD_ITEM(item)
  for (; item < nitems; item += stride) {
    uint4 kc[C::KSTEPS], qc[C::KSTEPS], vc[VN];
#pragma unroll
    for (int ks = 0; ks < C::KSTEPS; ++ks) {
      kc[ks] = kn[ks];
      qc[ks] = qn[ks];
    }
#pragma unroll
    for (int r = 0; r < VN; ++r) vc[r] = vn[r];
    const int h = (int)(item % heads);
    const int64_t bp = item / heads;
    const int64_t p = bp % positions, b = bp / positions;
    const int64_t qrow0 = b * qframes * positions + p;  // query / output row of frame 0
    if (item + stride < nitems) TM_LOAD_ITEM(item + stride)
    // ---- V chunks -> LDS image (d < D only)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // previous item's tr reads done
#pragma unroll
    for (int r = 0; r < VN; ++r) {
      const int idx = lane + 64 * r;
      const int f = idx / C::DCH, cc = idx - f * C::DCH;
      if (idx < frames * C::DCH) *(uint4*)(vl + f * C::VS + cc * 8) = vc[r];
    }
    // ---- S^T = K . Q^T
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < C::KSTEPS; ++ks)
      s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kc[ks]), __builtin_bit_cast(bf16x8, qc[ks]),
                                                  s, 0, 0, 0);
    // ---- softmax over keys 4*fq + j of query fr (log2 units)
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4 * fq + j >= frames) s[j] = -INFINITY;
      else if (!unitc) s[j] *= c;
      mx = fmaxf(mx, s[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pf[j] = (__bf16)__builtin_amdgcn_exp2f(s[j] - mx);
      pf[4 + j] = (__bf16)0.0f;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // V image written (the prefetch stays in flight)
    __builtin_amdgcn_wave_barrier();
    // ---- O^T = V^T . P^T, one 16-row block of d at a time
    f32x4 ot[C::DB];
#pragma unroll
    for (int a = 0; a < C::DB; ++a) {
      const bf16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (bf16x4 __attribute__((address_space(3)))*)(vl + vtr + 16 * a));
      const bf16x8 vf = {t[0], t[1], t[2], t[3], (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};
      ot[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    // row sum = O^T row D: block D/16, lane group (D%16)/4, element D%4
    const float l = __shfl(ot[D / 16][(D % 16) % 4], ((D % 16) / 4) * 16 + fr, 64);
    const float inv = __builtin_amdgcn_rcpf(l);
    if (qok) {
      bf16_t* orow = o + (qrow0 + (int64_t)fr * positions) * ldo + (int64_t)h * D;
#pragma unroll
      for (int a = 0; a < C::DB; ++a) {
        const int dd = 16 * a + 4 * fq;
        if (dd + 4 <= D)
          *(uint2*)(orow + dd) = make_uint2(pack2(ot[a][0] * inv, ot[a][1] * inv), pack2(ot[a][2] * inv, ot[a][3] * inv));
      }
    }
  }
#undef TM_LOAD_ITEM
}

// 17..32 frames (the DiT's 32-frame temporal blocks): the 16-frame kernel's scheme on two
// key blocks and two query blocks.  Per query block, S^T blocks (keys 16kb + 4fq + j,
// query 16qb + fr) give each lane 8 keys of its query; P^T's k-slot (fq, j) is key
// 4fq + j for j < 4 and 16 + 4fq + (j - 4) for j >= 4, and V^T's fragment takes the
// same keys from two tr reads 16 LDS rows apart, so one 16x16x32 MFMA per d-block sums
// all 32 keys.  The V^T fragments are read once per item and reused by both query blocks.
// ROPE (D = 64, the DiT's temporal blocks): the 1-D temporal RoPE of vd_rope_qk mode 1 is
// applied to the Q/K fragments as they are loaded — a lane's chunk at d-step 0 (dims
// 8fq..8fq+7) and d-step 1 (dims 32 + 8fq..) are exactly a rotate-half pair set, rotated
// by its frame f at angle f * theta^(-2i/64) in fp32 and rounded to bf16 as dit.hip's
// rope_kernel does — so the separate in-place RoPE pass over the Q/K rows disappears.
template <int D, bool ROPE = false>
__global__ __launch_bounds__(NT) void temporal_mfma32_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t ld,
    bf16_t* __restrict__ o, int64_t ldo, int64_t batch, int frames, int64_t positions, int heads,
    float c, float log2_theta) {
  static_assert(!ROPE || D == 64, "fused temporal RoPE: d = 64 only");
  using C = TmCfg<D>;
  __shared__ __attribute__((aligned(16))) bf16_t vimg[4][32 * C::VS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  bf16_t* vl = vimg[wave];
  for (int idx = lane; idx < 32 * C::VS / 8; idx += 64) *(uint4*)(vl + idx * 8) = make_uint4(0, 0, 0, 0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane < 32) vl[lane * C::VS + D] = (bf16_t)0x3F80;
  const int64_t nitems = batch * positions * heads;
  const int64_t stride = (int64_t)gridDim.x * 4;
  const bool unitc = c == 1.0f;
  const int vtr = (4 * fq + (fr >> 2)) * C::VS + 4 * (fr & 3);
  const int64_t lblk = xcd_remap(blockIdx.x, gridDim.x);
  for (int64_t item = lblk * 4 + wave; item < nitems; item += stride) {
    const int h = (int)(item % heads);
    const int64_t bp = item / heads;
    const int64_t p = bp % positions, b = bp / positions;
    const int64_t row0 = b * frames * positions + p;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // previous item's tr reads done
    for (int idx = lane; idx < frames * C::DCH; idx += 64) {
      const int f = idx / C::DCH, cc = idx - f * C::DCH;
      *(uint4*)(vl + f * C::VS + cc * 8) =
          *(const uint4*)(v + (row0 + (int64_t)f * positions) * ld + (int64_t)h * D + cc * 8);
    }
    // ---- S^T blocks: [qb][kb]
    f32x4 s[2][2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) s[qb][kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (ROPE) {
      uint4 kq[2][2], qq[2][2];  // [d-step][frame block]
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int f = 16 * t + fr;
          kq[ks][t] = qq[ks][t] = make_uint4(0, 0, 0, 0);
          if (f < frames) {
            const int64_t rf = (row0 + (int64_t)f * positions) * ld + (int64_t)h * D + ks * 32 + 8 * fq;
            kq[ks][t] = *(const uint4*)(k + rf);
            qq[ks][t] = *(const uint4*)(q + rf);
          }
        }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float pos = (float)(16 * t + fr);
        float ka[8], kb8[8], qa[8], qb8[8];
        unpack8(kq[0][t], ka); unpack8(kq[1][t], kb8);
        unpack8(qq[0][t], qa); unpack8(qq[1][t], qb8);
        float oka[8], okb[8], oqa[8], oqb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float inv_freq = exp2f(-log2_theta * (float)(2 * (8 * fq + j)) / (float)D);
          float sn, cs;
          __sincosf(pos * inv_freq, &sn, &cs);
          oka[j] = ka[j] * cs - kb8[j] * sn;
          okb[j] = kb8[j] * cs + ka[j] * sn;
          oqa[j] = qa[j] * cs - qb8[j] * sn;
          oqb[j] = qb8[j] * cs + qa[j] * sn;
        }
        kq[0][t] = pack8(oka); kq[1][t] = pack8(okb);
        qq[0][t] = pack8(oqa); qq[1][t] = pack8(oqb);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
            s[qb][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kq[ks][kb]),
                                                                __builtin_bit_cast(bf16x8, qq[ks][qb]), s[qb][kb], 0, 0,
                                                                0);
    } else {
#pragma unroll
    for (int ks = 0; ks < C::KSTEPS; ++ks) {
      const int dd = ks * 32 + 8 * fq;
      uint4 kq[2], qq[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int f = 16 * t + fr;
        kq[t] = qq[t] = make_uint4(0, 0, 0, 0);
        if (dd < D && f < frames) {
          const int64_t rf = (row0 + (int64_t)f * positions) * ld + (int64_t)h * D + dd;
          kq[t] = *(const uint4*)(k + rf);
          qq[t] = *(const uint4*)(q + rf);
        }
      }
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
          s[qb][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kq[kb]),
                                                              __builtin_bit_cast(bf16x8, qq[qb]), s[qb][kb], 0, 0, 0);
    }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // V image written
    __builtin_amdgcn_wave_barrier();
    bf16x8 vf[C::DB];
#pragma unroll
    for (int a = 0; a < C::DB; ++a) {
      const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (bf16x4 __attribute__((address_space(3)))*)(vl + vtr + 16 * a));
      const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (bf16x4 __attribute__((address_space(3)))*)(vl + 16 * C::VS + vtr + 16 * a));
      vf[a] = bf16x8{t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (16 * kb + 4 * fq + j >= frames) s[qb][kb][j] = -INFINITY;
          else if (!unitc) s[qb][kb][j] *= c;
          mx = fmaxf(mx, s[qb][kb][j]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      bf16x8 pf;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pf[j] = (__bf16)__builtin_amdgcn_exp2f(s[qb][0][j] - mx);
        pf[4 + j] = (__bf16)__builtin_amdgcn_exp2f(s[qb][1][j] - mx);
      }
      f32x4 ot[C::DB];
#pragma unroll
      for (int a = 0; a < C::DB; ++a)
        ot[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[a], pf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      const float l = __shfl(ot[D / 16][(D % 16) % 4], ((D % 16) / 4) * 16 + fr, 64);
      const float inv = __builtin_amdgcn_rcpf(l);
      const int f = 16 * qb + fr;
      if (f < frames) {
        bf16_t* orow = o + (row0 + (int64_t)f * positions) * ldo + (int64_t)h * D;
#pragma unroll
        for (int a = 0; a < C::DB; ++a) {
          const int dd = 16 * a + 4 * fq;
          if (dd + 4 <= D)
            *(uint2*)(orow + dd) = make_uint2(pack2(ot[a][0] * inv, ot[a][1] * inv), pack2(ot[a][2] * inv, ot[a][3] * inv));
        }
      }
    }
  }
}

// The head widths the MFMA kernels are instantiated for: calls f(integral_constant<int, D>) for
// the D among Ds that equals d (the callers have checked that one does).
template <int... Ds, typename F>
void with_d(int d, F f) {
  ((d == Ds ? f(std::integral_constant<int, Ds>{}) : (void)0), ...);
}

// items of 4 waves each, strided over at most 8192 workgroups
unsigned mfma_grid(int64_t items) {
  const int64_t g = (items + 3) / 4;
  return (unsigned)(g < 8192 ? g : 8192);
}

}  // namespace

static int temporal_entry(const void* q, const void* k, const void* v, int64_t ld, void* o, int64_t ldo,
                          int64_t batch, int32_t frames, int64_t positions, int32_t heads, int32_t d, float scale,
                          bool valu, vd_stream_t stream) {
  VD_CHECK_ARG(q && k && v && o && al16(q) && al16(k) && al16(v) && al16(o));
  VD_CHECK_ARG(ld % 8 == 0 && ldo % 8 == 0 && d % 8 == 0 && d > 0 && d <= 160);
  VD_CHECK_ARG(frames >= 1 && frames <= 32 && batch > 0 && positions > 0 && heads > 0);
  const int64_t items = batch * positions * heads;
  const unsigned grid = (unsigned)((items + 3) / 4);
  const float sl2 = scale * 1.4426950408889634f;
  hipStream_t s = (hipStream_t)stream;
  if (!valu && (d == 40 || d == 64 || d == 80 || d == 160 || (d == 32 && frames <= 16)) && ld % 8 == 0 &&
      ldo % 4 == 0) {
    const dim3 grid2(mfma_grid(items));
    if (frames <= 16)
      with_d<32, 40, 64, 80, 160>(d, [&](auto D) {
        hipLaunchKernelGGL(temporal_mfma_kernel<D()>, grid2, dim3(NT), 0, s, (const bf16_t*)q, ld, (const bf16_t*)k,
                           (const bf16_t*)v, ld, (bf16_t*)o, ldo, batch, frames, frames, positions, heads, sl2);
      });
    else
      with_d<40, 64, 80, 160>(d, [&](auto D) {
        hipLaunchKernelGGL(temporal_mfma32_kernel<D()>, grid2, dim3(NT), 0, s, (const bf16_t*)q, (const bf16_t*)k,
                           (const bf16_t*)v, ld, (bf16_t*)o, ldo, batch, frames, positions, heads, sl2, 0.f);
      });
    return vd_launch_status();
  }
  if (frames <= 8)
    hipLaunchKernelGGL(temporal_attn_kernel<8>, dim3(grid), dim3(NT), 0, s, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, ld, (bf16_t*)o, ldo, batch, frames,
                       positions, heads, d, sl2);
  else if (frames <= 16)
    hipLaunchKernelGGL(temporal_attn_kernel<16>, dim3(grid), dim3(NT), 0, s, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, ld, (bf16_t*)o, ldo, batch, frames,
                       positions, heads, d, sl2);
  else
    hipLaunchKernelGGL(temporal_attn_kernel<32>, dim3(grid), dim3(NT), 0, s, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, ld, (bf16_t*)o, ldo, batch, frames,
                       positions, heads, d, sl2);
  return vd_launch_status();
}

extern "C" int vd_temporal_attention(const void* q, const void* k, const void* v, int64_t ld,
                                     void* o, int64_t ldo, int64_t batch, int32_t frames,
                                     int64_t positions, int32_t heads, int32_t d, float scale,
                                     vd_stream_t stream) {
  return temporal_entry(q, k, v, ld, o, ldo, batch, frames, positions, heads, d, scale, false, stream);
}

extern "C" int vd_temporal_attention_valu(const void* q, const void* k, const void* v, int64_t ld,
                                          void* o, int64_t ldo, int64_t batch, int32_t frames,
                                          int64_t positions, int32_t heads, int32_t d, float scale,
                                          vd_stream_t stream) {
  return temporal_entry(q, k, v, ld, o, ldo, batch, frames, positions, heads, d, scale, true, stream);
}

extern "C" int vd_temporal_attention_kv(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                        void* o, int64_t ldo, int64_t batch, int32_t qframes, int32_t kframes,
                                        int64_t positions, int32_t heads, int32_t d, float scale,
                                        vd_stream_t stream) {
  VD_CHECK_ARG(q && k && v && o && al16(q) && al16(k) && al16(v) && al16(o));
  VD_CHECK_ARG(ldq % 8 == 0 && ldkv % 8 == 0 && ldo % 4 == 0);
  VD_CHECK_ARG(qframes >= 1 && qframes <= kframes && kframes <= 16 && batch > 0 && positions > 0 && heads > 0);
  if (!(d == 32 || d == 40 || d == 64 || d == 80 || d == 160)) return VD_EUNSUPPORTED;
  const dim3 grid(mfma_grid(batch * positions * heads));
  const float sl2 = scale * 1.4426950408889634f;
  hipStream_t s = (hipStream_t)stream;
  with_d<32, 40, 64, 80, 160>(d, [&](auto D) {
    hipLaunchKernelGGL(temporal_mfma_kernel<D()>, grid, dim3(NT), 0, s, (const bf16_t*)q, ldq, (const bf16_t*)k,
                       (const bf16_t*)v, ldkv, (bf16_t*)o, ldo, batch, qframes, kframes, positions, heads, sl2);
  });
  return vd_launch_status();
}

extern "C" int vd_temporal_attention_rope(const void* q, const void* k, const void* v, int64_t ld, void* o,
                                          int64_t ldo, int64_t batch, int32_t frames, int64_t positions,
                                          int32_t heads, int32_t d, float scale, float theta,
                                          vd_stream_t stream) {
  VD_CHECK_ARG(q && k && v && o && al16(q) && al16(k) && al16(v) && al16(o));
  VD_CHECK_ARG(ld % 8 == 0 && ldo % 4 == 0 && d == 64 && theta > 1.f);
  VD_CHECK_ARG(frames >= 17 && frames <= 32 && batch > 0 && positions > 0 && heads > 0);
  hipLaunchKernelGGL((temporal_mfma32_kernel<64, true>), dim3(mfma_grid(batch * positions * heads)), dim3(NT), 0,
                     (hipStream_t)stream, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld, (bf16_t*)o, ldo,
                     batch, frames, positions, heads, scale * 1.4426950408889634f, log2f(theta));
  return vd_launch_status();
}
