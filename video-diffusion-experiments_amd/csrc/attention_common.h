// What more than one attention translation unit uses: tile constants, the cross-lane and
// staging helpers shared by the flash kernels, flash32's configuration (flash40 runs its
// arithmetic), the LDS-DMA helpers of flash40 / flash80, and the host-side plan and operand
// structs that attention.hip hands to each family's launch function.  Everything here has
// internal or hidden linkage; a kernel instance lives in exactly one attention_*.hip.
#pragma once
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int KT = 64;   // keys per tile

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Cross-lane max over the 4 lanes holding one query (l, l^16, l^32, l^48):
// v_permlane32_swap / v_permlane16_swap + max, no LDS traffic (T12).
__device__ __forceinline__ float max_over_query_lanes(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  auto t = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(t[0]), __uint_as_float(t[1]));
}

// K/V tile staging: the in-flight tile lives in one ext_vector register block
// (4 dwords per 16-byte chunk) with compile-time element indices — arrays of
// uint4 passed around were left as a scratch stack object by the compiler.
template <int L>
using stage_t = __attribute__((ext_vector_type(8 * L))) uint32_t;  // K chunks then V chunks

// One tile of up to KT keys starting at row key0; rows past kmax (the tile's last valid row) are
// clamped to it.
template <int L>
__device__ __forceinline__ stage_t<L> kv_load_rows(const bf16_t* kb_ptr, const bf16_t* vb_ptr, int ldk,
                                                   int ldv, int64_t key0, int kmax, const int (&krow)[L],
                                                   const uint32_t (&kcol)[L]) {
  const bf16_t* kp = kb_ptr + key0 * ldk;
  const bf16_t* vp = vb_ptr + key0 * ldv;
  stage_t<L> st;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int r = krow[i] < kmax ? krow[i] : kmax;
    const uint4 a = *(const uint4*)(kp + (uint32_t)(r * ldk) + kcol[i]);
    const uint4 b = *(const uint4*)(vp + (uint32_t)(r * ldv) + kcol[i]);
    st[4 * i + 0] = a.x; st[4 * i + 1] = a.y; st[4 * i + 2] = a.z; st[4 * i + 3] = a.w;
    st[4 * L + 4 * i + 0] = b.x; st[4 * L + 4 * i + 1] = b.y;
    st[4 * L + 4 * i + 2] = b.z; st[4 * L + 4 * i + 3] = b.w;
  }
  return st;
}
template <int L>
__device__ __forceinline__ stage_t<L> kv_load(const bf16_t* kb_ptr, const bf16_t* vb_ptr, int ldk,
                                              int ldv, int t, int64_t skv, const int (&krow)[L],
                                              const uint32_t (&kcol)[L]) {
  const int64_t key0 = (int64_t)t * KT;
  // kmax >= KT-1 except on a ragged last tile
  return kv_load_rows<L>(kb_ptr, vb_ptr, ldk, ldv, key0, (int)(skv - 1 - key0), krow, kcol);
}

// flash32's tile configuration (flash40 runs the same arithmetic at D = 40).
template <int D>
struct F32Cfg {
  static_assert(D % 8 == 0 && D <= 48, "flash32: d must be a multiple of 8, <= 48");
  static constexpr int DK = (D + 1 + 15) / 16 * 16;   // contraction incl. the -mu column
  static constexpr int KSTEPS = DK / 16;
  static constexpr int DVP = (D + 1 + 31) / 32 * 32;  // PV rows incl. the ones column
  static constexpr int NDB = DVP / 32;
  static constexpr int KS = DK + 8;                   // K LDS row (elements), conflict-free
  static constexpr int DCH = D / 8;                   // 16-B chunks per K/V row
  static constexpr int K_ELEMS = KT * KS;
  static constexpr int V_ELEMS = NDB * KT * 32;
  static constexpr int STAGE = K_ELEMS + V_ELEMS;     // elements per buffer
  static constexpr int LREG = (KT * DCH + NT - 1) / NT;
  // position of d = D in the Q'^T fragment (k-step, lane half, element)
  static constexpr int MU_KS = D / 16, MU_H = (D % 16) / 8, MU_J = D % 8;
  // position of the ones column in the O^T accumulator (d-block, lane half, register)
  static constexpr int L_DB = D / 32, L_H = ((D % 32) / 4) & 1, L_I = (D % 4) + 4 * ((D % 32) / 8);
};

constexpr float F32_THR = 6.0f;  // deferred-max threshold (log2 units): P <= 64
constexpr int F32_FIXW = 16;     // blocks per workgroup of flash32's exact fix-up pass (attention_flash32.hip)

__device__ __forceinline__ float vmax3(float a, float b, float c) {
  // plain v_max3_f32: fmaxf would add IEEE canonicalising maxes on MFMA results
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float vmax2(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// max over the 32 scores a lane holds for its query in one 64-key tile
__device__ __forceinline__ float tile_max(const f32x16& a, const f32x16& b) {
  float m0 = vmax3(a[0], a[1], a[2]), m1 = vmax3(a[3], a[4], a[5]), m2 = vmax3(a[6], a[7], a[8]);
  float m3 = vmax3(a[9], a[10], a[11]), m4 = vmax3(a[12], a[13], a[14]), m5 = vmax3(a[15], b[0], b[1]);
  float m6 = vmax3(b[2], b[3], b[4]), m7 = vmax3(b[5], b[6], b[7]), m8 = vmax3(b[8], b[9], b[10]);
  float m9 = vmax3(b[11], b[12], b[13]), m10 = vmax2(b[14], b[15]);
  m0 = vmax3(m0, m1, m2);
  m3 = vmax3(m3, m4, m5);
  m6 = vmax3(m6, m7, m8);
  m9 = vmax2(m9, m10);
  return vmax2(vmax3(m0, m3, m6), m9);
}
// value of lane l ^ 32 (v_permlane32_swap)
__device__ __forceinline__ float partner32(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  // r[0] = new vdst (lanes 32-63 <- src of lanes 0-31), r[1] = new src (lanes 0-31 <- vdst of lanes 32-63)
  return __uint_as_float((threadIdx.x & 32) ? r[0] : r[1]);
}

// flash40 / flash80: workgroup shape and the LDS-DMA ring (attention_flash40.hip, attention_flash80.hip)
constexpr int F4_NW = 8, F4_NT = 512, F4_QB = 2, F4_QWG = F4_NW * 32 * F4_QB;
constexpr int F4_RING = 4;
constexpr int F8K_QWG = F4_NW * 32;  // flash80: queries per workgroup

__device__ const uint32_t f4_ones[4] = {0x3F80u, 0u, 0u, 0u};  // bf16 {1, 0 x 7}: the ones chunks

__device__ __forceinline__ u32x4 f4_rsrc(const void* base, uint32_t bytes) {
  const uint64_t a = (uint64_t)base;
  u32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((uint32_t)a);
  r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) & 0xffffu;  // stride 0
  r[2] = __builtin_amdgcn_readfirstlane(bytes);                          // num_records: range check
  r[3] = 0x00020000u;
  return r;
}

// One 1 KiB LDS-DMA piece: lane l's 16 bytes at voff land at LDS byte lds + 16 l.  Inline asm:
// M0 written in the statement that reads it, and hipcc does not count it in vmcnt (f4_wait_vm).
__device__ __forceinline__ void f4_dma(u32x4 rs, uint32_t lds, uint32_t voff) {
  uint32_t keep;
  asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
               "buffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(lds), "v"(voff), "s"(rs) : "memory");
}

// Pin a value at this point of the instruction stream: hipcc's sinking passes otherwise move
// the V phase's exp2/packs (pure register work) past the s_barrier into the M phase, next to
// the MFMAs that use them, which undoes the ping-pong.  Never pin an MFMA result: hipcc pads no
// wait states for an asm reader, and after the asm it takes the register as the asm's output, so
// the later VALU readers lose their MFMA hazard padding (a race with the still-running MFMA).
template <typename T>
__device__ __forceinline__ void f4_pin(T& x) {
  asm volatile("" : "+v"(x));
}

template <int N>
__device__ __forceinline__ void f4_wait_vm() {
  if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void f4_bar() {  // this wave's LDS reads drained, DMA left in flight
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

}  // namespace

namespace vdattn __attribute__((visibility("hidden"))) {

// The operands of one attention call, as every flash kernel takes them (c = scale * log2 e).
struct Args {
  const bf16_t *q, *k, *v;
  bf16_t* o;
  int64_t ldq, ldk, ldv, ldo, batch;
  int heads;
  int64_t sq, skv, kv_div;
  float c;
  int out_f32;
  hipStream_t s;
};

// What a call runs (attention.hip: plan()); the launch functions execute it and decide nothing.
struct Plan {
  int rc;            // VD_OK, or the refusal (VD_EINVAL / VD_EUNSUPPORTED) with every other field 0
  int family;        // VD_ATTN_K_*
  int qblk;          // 16-query blocks per wave of the 16x16x32 flash kernel (2 or 4), 0 elsewhere
  bool unitc;        // flash32 / flash40 / flash80: the c == 1 instance (no per-score multiply)
  bool causal;       // VD_ATTN_CAUSAL
  int tail;          // VD_ATTN_TAIL(n): n, else 0
  int64_t grid;      // workgroups of the (first) launch
  int64_t fix_grid;  // flash40: workgroups of the exact pass launched after it, else 0
};

// Launch kern over grid x threads with the 14 operands every flash kernel starts with, then `extra`.
template <typename... Ps, typename... Extra>
inline int launch(void (*kern)(Ps...), dim3 grid, int threads, const Args& a, Extra... extra) {
  hipLaunchKernelGGL(kern, grid, dim3(threads), 0, a.s, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, a.o, a.ldo, a.heads, a.sq,
                     a.skv, a.kv_div, a.c, a.out_f32, extra...);
  return vd_launch_status();
}

int launch_flash(int d, const Args& a, const Plan& p);   // attention_flash.hip
int launch_flash32(const Args& a, const Plan& p);        // attention_flash32.hip (d = 40)
int launch_flash32_exact(const Args& a, const Plan& p);  //   flash40's exact pass, p.fix_grid workgroups
int launch_flash40(const Args& a, const Plan& p);        // attention_flash40.hip, then the exact pass
int launch_flash80(const Args& a, const Plan& p);        // attention_flash80.hip
int launch_flash512(const Args& a, const Plan& p);       // attention_d512.hip

}  // namespace vdattn
