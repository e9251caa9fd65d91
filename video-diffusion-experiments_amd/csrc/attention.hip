// Attention for gfx950: the host side.  One kernel family per file, what they share in
// attention_common.h; this file decides which one a call runs (plan) and runs it (dispatch).
//
//   attention_flash.hip     flash_attn_kernel, v_mfma_f32_16x16x32_bf16: every head width
//                           (d = 32 / 40 / 64 / 80 / 128 / 160), the causal instances (CLIP) and the
//                           tailed ones (IP-Adapter).  4 waves x 16 QBLK queries, QBLK 2 or 4.
//   attention_flash32.hip   flash32, v_mfma_f32_32x32x16_bf16 at d = 40: the short and the text
//                           cross-attention of level 1, and the exact pass that follows flash40.
//   attention_flash40.hip   flash40: d = 40 from 4 key tiles (the level-1 self-attention), flash32's
//                           arithmetic as a two-group ping-pong over an LDS-DMA ring.
//   attention_flash80.hip   flash80: d = 80 from 4 key tiles (level 2) on flash40's schedule.
//   attention_d512.hip      flash512: the VAE mid block's single 512-wide head (and the row
//                           softmax of its earlier materialised form).
//   attention_temporal.hip  the motion module's attention over frames; entry points of its own.
//   attention_fp8.hip       the DiT's fp8 attention; entry points of its own.
#include "attention_common.h"

using vdattn::Args;
using vdattn::Plan;

namespace {

// What vd_attention_ex would run, from the sizes, the output's address and stride, and the
// kernel word alone: no operand is read, nothing is launched.  kernel's low byte: 0 = automatic
// (d = 40: flash40 from 4 key tiles, flash32 below; d = 80: flash80 from 4 key tiles; else the
// 16x16x32 flash kernel), 1 = the 16x16x32 flash kernel, 2 = flash32 (d = 40), 3 = flash40 /
// flash80 (d = 40 / 80) from 2 key tiles.  A forced kernel that does not take the shape falls
// through to the next one down, and the plan says so; causal and tailed calls always run the
// 16x16x32 flash kernel.
Plan plan(int d, int64_t sq, int64_t skv, int64_t batch, int heads, int64_t kv_div, const void* o, int64_t ldo,
          int out_f32, int kernel, float scale) {
  const auto refuse = [](int rc) {
    Plan r{};
    r.rc = rc;
    return r;
  };
  if (!(o && ((uintptr_t)o & 7) == 0 && ldo % 4 == 0 && (!out_f32 || al16(o)))) return refuse(VD_EINVAL);
  if (!(batch > 0 && heads > 0 && sq > 0 && skv > 0 && kv_div > 0 && batch % kv_div == 0)) return refuse(VD_EINVAL);
  if (!(batch <= 65535 && heads <= 65535)) return refuse(VD_EINVAL);
  if (!(kernel >= 0 && (kernel & ~(0xff | VD_ATTN_CAUSAL | VD_ATTN_TAIL_MASK)) == 0 && (kernel & 0xff) <= 3))
    return refuse(VD_EINVAL);
  const int forced = kernel & 0xff;
  const bool causal = (kernel & VD_ATTN_CAUSAL) != 0;
  const int tail = (kernel & VD_ATTN_TAIL_MASK) >> VD_ATTN_TAIL_SHIFT;
  if (tail && !(tail <= KT && tail < skv && !causal && scale > 0.f)) return refuse(VD_EINVAL);
  if (!tail && causal && !(sq == skv && kv_div == 1 && scale > 0.f)) return refuse(VD_EINVAL);

  const bool plain = !tail && !causal;
  if (tail ? !(d == 32 || d == 40 || d == 64 || d == 80 || d == 160)
           : causal ? !(d == 32 || d == 64)
                    : !(d == 32 || d == 40 || d == 64 || d == 80 || d == 128 || d == 160 || d == 512))
    return refuse(VD_EUNSUPPORTED);

  // 16-byte output rows: the stores of every kernel but the 16x16x32 one
  const bool oal = al16(o) && ldo % (out_f32 ? 4 : 8) == 0;
  const bool ring = forced == 3 || (forced == 0 && skv >= 4 * KT);  // flash40 / flash80 wanted ...
  Plan p{};
  int64_t qwg;  // queries per workgroup
  if (d == 512) {
    if (!oal) return refuse(VD_EINVAL);
    p.family = VD_ATTN_K_FLASH512;
    qwg = 128;
  } else if (plain && d == 40 && ring && skv >= 2 * KT && oal) {   // ... and taken from 2 key tiles
    p.family = VD_ATTN_K_FLASH40;
    qwg = F4_QWG;
  } else if (plain && d == 40 && forced != 1 && oal) {
    p.family = VD_ATTN_K_FLASH32;
    qwg = 256;
  } else if (plain && d == 80 && ring && skv >= 2 * KT && oal) {
    p.family = VD_ATTN_K_FLASH80;
    qwg = F8K_QWG;
  } else {
    p.family = VD_ATTN_K_FLASH;
    p.qblk = d <= 40 && sq >= 1024 ? 4 : 2;
    qwg = 64 * p.qblk;
  }
  p.grid = (sq + qwg - 1) / qwg * heads * batch;
  // the 16x16x32 kernel's grid is (query blocks, heads, batch); the others' is one dimension
  if (p.family != VD_ATTN_K_FLASH && p.grid > 0x7fffffff) return refuse(VD_EINVAL);
  if (p.family == VD_ATTN_K_FLASH40)  // the exact pass: 128-query blocks, F32_FIXW per workgroup
    p.fix_grid = ((sq + 127) / 128 * heads * batch + F32_FIXW - 1) / F32_FIXW;
  p.unitc = (p.family == VD_ATTN_K_FLASH32 || p.family == VD_ATTN_K_FLASH40 || p.family == VD_ATTN_K_FLASH80) &&
            scale * 1.4426950408889634f == 1.0f;
  p.causal = causal;
  p.tail = tail;
  p.rc = VD_OK;
  return p;
}

int attention_entry(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                    int64_t ldo, int64_t batch, int32_t heads, int64_t sq, int64_t skv, int32_t d, int64_t kv_div,
                    float scale, vd_stream_t stream, int out_f32, int kernel) {
  VD_CHECK_ARG(q && k && v && al16(q) && al16(k) && al16(v));
  VD_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0);
  const Plan p = plan(d, sq, skv, batch, heads, kv_div, o, ldo, out_f32, kernel, scale);
  if (p.rc == VD_EINVAL) return p.rc;
  VD_CHECK_ARG(skv * ldk < 0x7fffffff && skv * ldv < 0x7fffffff);
  if (p.rc != VD_OK) return p.rc;
  const Args a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, ldq, ldk, ldv, ldo, batch, heads,
               sq, skv, kv_div, scale * 1.4426950408889634f, out_f32, (hipStream_t)stream};
  switch (p.family) {
    case VD_ATTN_K_FLASH: return vdattn::launch_flash(d, a, p);
    case VD_ATTN_K_FLASH32: return vdattn::launch_flash32(a, p);
    case VD_ATTN_K_FLASH40: return vdattn::launch_flash40(a, p);
    case VD_ATTN_K_FLASH80: return vdattn::launch_flash80(a, p);
    default: return vdattn::launch_flash512(a, p);
  }
}

}  // namespace

extern "C" int vd_attention_plan(const void* o, int64_t ldo, int64_t batch, int32_t heads, int64_t sq, int64_t skv,
                                 int32_t d, int64_t kv_div, float scale, int32_t out_f32, int32_t kernel,
                                 int32_t* family, int32_t* qblk, int32_t* unit_scale, int64_t* grid,
                                 int64_t* exact_grid) {
  VD_CHECK_ARG(family && qblk && unit_scale && grid && exact_grid);
  const Plan p = plan(d, sq, skv, batch, heads, kv_div, o, ldo, out_f32 != 0, kernel, scale);
  *family = p.family;
  *qblk = p.qblk;
  *unit_scale = p.unitc;
  *grid = p.grid;
  *exact_grid = p.fix_grid;
  return p.rc;
}

extern "C" int vd_attention(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                            int64_t ldv, void* o, int64_t ldo, int64_t batch, int32_t heads,
                            int64_t sq, int64_t skv, int32_t d, int64_t kv_div, float scale,
                            vd_stream_t stream) {
  return attention_entry(q, ldq, k, ldk, v, ldv, o, ldo, batch, heads, sq, skv, d, kv_div, scale, stream, 0, 0);
}

extern "C" int vd_attention_f32(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                int64_t ldv, float* o, int64_t ldo, int64_t batch, int32_t heads,
                                int64_t sq, int64_t skv, int32_t d, int64_t kv_div, float scale,
                                vd_stream_t stream) {
  return attention_entry(q, ldq, k, ldk, v, ldv, o, ldo, batch, heads, sq, skv, d, kv_div, scale, stream, 1, 0);
}

extern "C" int vd_attention_ex(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                               int64_t ldv, void* o, int64_t ldo, int64_t batch, int32_t heads, int64_t sq,
                               int64_t skv, int32_t d, int64_t kv_div, float scale, int32_t out_f32,
                               int32_t kernel, vd_stream_t stream) {
  return attention_entry(q, ldq, k, ldk, v, ldv, o, ldo, batch, heads, sq, skv, d, kv_div, scale, stream,
                         out_f32 != 0, kernel);
}
