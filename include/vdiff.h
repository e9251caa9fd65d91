/*
 * vdiff.h — C ABI of libvdiff_hip.so, the MI355X (gfx950) kernels behind the
 * video-diffusion denoising step.
 *
 * The reference has no native code: every op below replaces a stock
 * torch/cuDNN/cuBLAS/SDPA call that diffusers issues inside
 * `UNetMotionModel.forward` (called at
 * /root/reference/experiments/03_trace_forward_pass.py:109-113) and
 * `DDIMScheduler.step` (configured at
 * /root/reference/experiments/05_grid_search_ablation.py:136-141, stepped
 * inside the pipe(...) call at :158-167).  Per-entry citations name the
 * diffusers op replaced.
 *
 * Conventions:
 *  - plain device pointers + explicit int64 sizes/strides (in ELEMENTS);
 *  - activations bf16 ("bf16" = raw 16-bit storage), statistics and
 *    latents fp32, weights bf16 packed [N][K] (K contiguous);
 *  - every call takes the hipStream_t to launch on, never allocates, never
 *    synchronises, never retains a pointer: all calls are hipGraph-capturable;
 *  - returns 0 (VD_OK) or a vd_status / hipError_t code; vd_strerror() names it.
 *  - activation layout is NHWC rows: pixel/token m of image n at row
 *    n*H*W + h*W + w; video b, frame f -> image n = b*F + f.
 */
#ifndef VDIFF_H
#define VDIFF_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vd_stream_t; /* hipStream_t */

enum vd_status {
  VD_OK = 0,
  VD_EINVAL = 1000,       /* bad shape / alignment / unsupported parameter */
  VD_EUNSUPPORTED = 1001, /* valid request outside the compiled variants    */
  VD_ERCCL = 1002         /* RCCL call failed                                */
};

const char* vd_strerror(int code);
int vd_version(void);  /* 6 */
/* Content hash (16 hex digits) of the sources and compile flags the library was built from
 * (video-diffusion-experiments_amd/build_ext.py); the Python loader compares it with the tree. */
const char* vd_build_hash(void);
/* The --offload-arch the library's code objects were compiled for ("gfx950" unless the build
 * set VDIFF_ARCH); not part of the content hash above. */
const char* vd_build_arch(void);

/* ---------------------------------------------------------------- GEMM / conv
 * out[m, n] = epi( sum_k A[m, k] * W[n, k] )          (bf16 MFMA, fp32 accumulate)
 *
 * a_mode VD_A_DENSE : A[m, k] = a0[m*lda0 + k]              for k <  k0
 *                              a1[m*lda1 + (k - k0)]       for k >= k0  (channel concat)
 * a_mode VD_A_CONV3X3: implicit-GEMM 3x3 conv, pad 1, over NHWC images (or a kt x 3 x 3
 *   conv over the frames of each video, see kt below); the
 *   K index is tap*(Cin) + ci with Cin = k0 + (channels of a1); channels
 *   [0,k0) come from a0 (pixel stride lda0), the rest from a1 (pixel stride
 *   lda1) — this is the up-block torch.cat([x, skip], 1) without materialising
 *   it.  stride 2 = Downsample2D; upsample 1 = Upsample2D (nearest x2 of the
 *   h_in x w_in input, then conv).  M = n_img*h_out*w_out.
 *   stride 2 | VD_CONV_PAD_END = the VAE encoder's Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1))
 *   then a 3x3 stride-2 conv without padding — taps at input row 2*oh + dy, column 2*ow + dx
 *   (dy, dx in 0..2), zero where that is >= h_in / w_in, so the zero band is at the far edge only.
 *   h_out = (h_in - 2) / 2 + 1 and w_out alike (the pad-1 size for even inputs, one less for odd
 *   ones).  The flag rides in `stride` because the struct cannot grow (its tail is pinned); it is
 *   legal only as 2 | VD_CONV_PAD_END with kt <= 1, ks in {0, 3} and upsample 0, and any other
 *   bit of `stride` above the low byte is VD_EINVAL.  The plan (kernel, split, workspace) is that
 *   of plain stride 2.
 *   Replaces torch conv2d in ResnetBlock2D.conv1/conv2, Down/Upsample2D.conv,
 *   conv_in/conv_out and nn.Linear / 1x1 convs (a5, a8, a10).
 * epilogue, in order: + bias[n] (fp32) ; + rowbias[(m / rb_div) * ld_rb + n]
 *   (fp32, the ResnetBlock2D time_emb_proj broadcast) ; act ; + res[m*ld_res + n]
 *   (bf16) ; store bf16 (or fp32 if out_f32).
 * act VD_ACT_GEGLU: W rows are packed in 16-row blocks alternating (hidden,
 *   gate); out has N/2 columns: h * gelu_erf(g)  (diffusers GEGLU, a10).
 */
enum { VD_A_DENSE = 0, VD_A_CONV3X3 = 1 };
enum { VD_CONV_PAD_END = 0x100 }; /* OR-ed into vd_gemm_desc.stride, see above */
enum { VD_ACT_NONE = 0, VD_ACT_SILU = 1, VD_ACT_GEGLU = 2, VD_ACT_GELU = 3, VD_ACT_QUICK_GELU = 4 };
/* VD_ACT_GELU: pointwise gelu (erf form) — the DiT MLP (build-defined, §8f rank 3).
 * VD_ACT_QUICK_GELU: x * sigmoid(1.702 x) in fp32 — the CLIP text encoder's MLP (SD-1.5's
 * hidden_act "quick_gelu"); planned exactly as VD_ACT_GELU. */

typedef struct vd_gemm_desc {
  const void* a0; int64_t lda0; int64_t k0;
  const void* a1; int64_t lda1;
  int32_t a_mode;
  int32_t n_img, h_in, w_in, h_out, w_out, stride, upsample;
  const void* w; int64_t ldw;
  int64_t M, N, K;
  const float* bias;
  const float* rowbias; int64_t ld_rb; int64_t rb_div;
  const void* res; int64_t ld_res;
  int32_t act;
  void* out; int64_t ldc; int32_t out_f32;
  /* split-K workspace (fp32 partial slabs); size from vd_gemm_ws_bytes(), may be
   * NULL when that returns 0. */
  void* ws; int64_t ws_bytes;
  /* 3-D / (2+1)D conv (VD_A_CONV3X3 only): a kt x ks x ks kernel over the frames of each
   * video — kt temporal taps (1 or 3; 0 means 1), ks spatial (3, or 1 for the temporal half
   * of a (2+1)D conv; 0 means 3; pad ks/2).  K index = (dt*ks*ks + tap)*Cin + ci.  Output
   * image n = b*frames_out + f reads, at temporal tap dt, input image
   * b*frames_in + f + t_off + dt - kt/2, zero outside [0, frames_in) (the conv's temporal
   * zero padding; a frame-sharded rank passes its halo'd frames with frames_in =
   * frames_out + 2, t_off = 1).  n_img counts OUTPUT images. */
  int32_t kt, ks, frames_in, frames_out, t_off;
  /* Fused LayerNorm of the output rows (BasicTransformerBlock norm1/2/3 after the GEMM that
   * produces the residual stream: proj_in, attn out-proj + residual): when ln_out != NULL,
   * also ln_out[m] = (out[m] - mean) * rstd * ln_gamma + ln_beta
   * (+ ln_pe[((m / ln_pe_div) % ln_pe_period) * N .. ], the motion block's sinusoidal PE),
   * statistics over the N bf16-rounded outputs of row m (vd_layernorm's arithmetic).  Fused
   * into the 256 x 320 GEMM's epilogue when N == 320 (one tile owns whole rows); otherwise
   * vd_gemm runs vd_layernorm on the output after the GEMM.  bf16 outputs only. */
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  const float* ln_pe; int64_t ln_pe_div; int64_t ln_pe_period;
  void* ln_out; int64_t ld_ln;
  /* Per-call plan controls (the library keeps no mutable selector state; zero = the product
   * plan).  path: 0 = automatic; 1 = v1 (register-staged, any shape), 2 = v2 (256 x {128,160}
   * persistent LDS-DMA), 3 = v3 (256 x 256 ping-pong, dense A), 5 = v5 (256 x 320, BK 32),
   * 6 = v6 (64 x 64, split K toward 2 workgroups per CU), 8 = v8 (weight-stationary, dense
   * K = 320, M >= 4096; automatic at M >= 16384), 9 = v9 (M <= 16 rows: one wave per 16
   * columns streaming W, v1's arithmetic; never automatic since round 6) — forced wherever that kernel takes the
   * shape, else the automatic choice; every path computes the same arithmetic for an
   * unsplit K (the K order of each output is fixed), the parity tests run each one.
   * plan_m > 0: choose kernel, split-K and LayerNorm fusion as if M were plan_m, launch over
   * all M rows — an unsharded run planned with a frame shard's M reproduces the shard's
   * summation order bit for bit (tests/test_gpu_dist2.py). */
  int32_t path;
  int64_t plan_m;
  /* Output-row permutation (round 5; 0 = none): with rmap_inner > 0 the epilogue writes row m
   * of the product — and reads its residual — at row rev3(m), where
   *   m = ((i0*rmap_n1 + i1)*rmap_n2 + i2)*rmap_inner + j  ->  ((i2*rmap_n1 + i1)*n0 + i0)*rmap_inner + j,
   * n0 = M / (rmap_n1*rmap_n2*rmap_inner).  The frame-sharded motion module's proj_out takes the
   * rows of the returning all-to-all, (position chunk, frame, video, position) on a rank, and writes
   * them straight into the rank's (video, frame, position) layout with the residual added
   * (vdiff.dist.FrameShard.return_perm) — no separate re-shard transpose.  Not with ln_out, GEGLU
   * or a row bias. */
  int32_t rmap_n1, rmap_n2, rmap_inner;
  /* LayerNorm folded into the consuming GEMM (round 5; NULL = none).  With ln_fold_s != NULL
   * the A rows are the UN-normalised LayerNorm input x (K = its row length), w = W∘gamma (each
   * column k of the Linear's W scaled by gamma[k], rounded to bf16 once), bias = b + W·beta
   * (fp32), and ln_fold_s[n] = Σ_k w[n][k] in fp32 (of the bf16 w).  The kernel takes each row's
   * mean and rstd = 1/sqrt(var + ln_fold_eps) from A itself (Σx and Σx² over the A fragments it
   * holds: two extra MFMAs per X fragment, on v8 and v6) and its epilogue forms
   *   rstd·(Σ_k w[n][k] x[m][k] − mean·ln_fold_s[n]) + bias[n]   (then act / GEGLU as usual)
   * = Linear(LayerNorm(x)) without the normalised rows being written or read.  Only the
   * weight-stationary v8 path (K = 320) and an unsplit v6 (levels 2-4 of a rank) carry it (dense, no
   * residual / rmap; a row bias — the motion block's positional encoding W·pe[frame] — is added
   * after the fold on v6): vd_gemm_plan reports kernel 0 and vd_gemm returns
   * VD_EUNSUPPORTED for any other plan. */
  const float* ln_fold_s; float ln_fold_eps;
} vd_gemm_desc;

int vd_gemm(const vd_gemm_desc* d, vd_stream_t stream);
/* The plan vd_gemm would run for this descriptor (its path / plan_m controls included):
 * *kernel = 1, 2, 3, 5, 6 or 8 (v1 .. v8; 0: no kernel takes it, vd_gemm would refuse it) and
 * *split = its K slices.  Lets a caller choose between a folded and an unfolded form (ln_fold_s)
 * and lets tools label their timings; no launch, no state. */
int vd_gemm_plan(const vd_gemm_desc* d, int32_t* kernel, int32_t* split);
/* Workspace bytes vd_gemm needs for this descriptor (0 = none): shapes with too
 * few output tiles to fill 256 CUs are split along K into fp32 slabs that a
 * second kernel reduces (deterministic, no atomics) while applying the epilogue. */
int64_t vd_gemm_ws_bytes(const vd_gemm_desc* d);
/* The 64 x 64 level's FeedForward in one launch (csrc/ff.hip; C = 320, hidden = 1280 only, else
 * VD_EUNSUPPORTED; any M >= 1):
 *   out[m] = res[m] + b2 + W2 · bf16((h + bh) · gelu_erf(g + bg)),  [h | g] = W1' · x[m]
 * x bf16 [M][C] rows (row stride ldx), w1 the GEGLU projection packed as vd_gemm's VD_ACT_GEGLU
 * takes it ([2 hidden][C]: 16-row blocks hidden i, gate i, ...; contiguous), b1 fp32 [2 hidden] in the
 * same order or NULL, w2 bf16 [C][hidden] contiguous, b2 fp32 [C] or NULL, res bf16 rows (ld_res) or
 * NULL, out bf16 rows (ldc).  ln_fold_s != NULL folds the LayerNorm of x's rows into the GEGLU
 * projection exactly as vd_gemm_desc.ln_fold_s does (w1 = W∘gamma, b1 = b + W·beta, ln_fold_s its
 * fp32 row sums).  The hidden activation is never written; the output bits equal
 * vd_gemm(VD_ACT_GEGLU) followed by vd_gemm(res) as planned for M = 131072 rows, and a row's result
 * does not depend on M.  vd_ff_fused_takes: 1 where the product plan runs the fused launch in place
 * of the two (C = 320, hidden = 4C, M >= 65536), else 0; no launch, no state.  It is asked about
 * the shape alone: operands vd_ff_fused cannot address (row strides with M * ld * 2 >= 2^31 bytes,
 * unaligned pointers, strides not a multiple of 8) are VD_EINVAL there, and such a caller runs
 * the two vd_gemm launches itself. */
int vd_ff_fused(const void* x, int64_t ldx, int64_t M, int64_t C, int64_t hidden, const void* w1,
                const float* b1, const float* ln_fold_s, float ln_eps, const void* w2, const float* b2,
                const void* res, int64_t ld_res, void* out, int64_t ldc, vd_stream_t stream);
int vd_ff_fused_takes(int64_t M, int64_t C, int64_t hidden);
/* ---------------------------------------------------------------- GroupNorm
 * torch GroupNorm over NHWC rows, for ResnetBlock2D.norm1/2 (eps 1e-5, +SiLU),
 * Transformer2DModel.norm (eps 1e-6) and the motion-module norm whose
 * statistics span (C/G, F, H, W) (eps 1e-6) — SURVEY.md §8a a11.
 * An "instance" is a run of pix_per_inst consecutive NHWC rows sharing
 * statistics (one image, or all F frames of a video).  Channels [0,c0) come
 * from x0 (row stride ldx0), [c0,C) from x1 (row stride ldx1).
 *   vd_gn_partial : per (inst, split, channel) {count, mean, M2, 0} -> ws
 *                   ws has n_inst*n_split*C float4 entries.
 *   vd_gn_finalize: combines n_split_total partial splits (Chan), groups of
 *                   C/groups channels, -> scale_shift[inst][C] float2 {a, b}
 *                   with y = x*a + b = (x-mean)*rstd*gamma + beta.
 *   vd_gn_apply   : y = x*a + b (then SiLU if silu) -> bf16 rows (ldy).
 */
int vd_gn_partial(const void* x0, int64_t ldx0, int64_t c0, const void* x1, int64_t ldx1,
                  int64_t C, int64_t n_inst, int64_t pix_per_inst, int32_t n_split,
                  float* ws, vd_stream_t stream);
int vd_gn_finalize(const float* ws, int64_t n_inst, int32_t n_split_total, int64_t C,
                   int32_t groups, float eps, const float* gamma, const float* beta,
                   float* scale_shift, vd_stream_t stream);
int vd_gn_apply(const void* x0, int64_t ldx0, int64_t c0, const void* x1, int64_t ldx1,
                int64_t C, int64_t n_inst, int64_t pix_per_inst, const float* scale_shift,
                int32_t silu, void* y, int64_t ldy, vd_stream_t stream);
/* vd_gn_apply writing input row m to output row rev3(m) (the vd_gemm_desc.rmap_* map: rows
 * ((i0*n1 + i1)*n2 + i2)*inner + j -> ((i2*n1 + i1)*n0 + i0)*inner + j; n1, n2, inner powers of
 * two, inner = 0 the identity): the frame-sharded motion module's norm writes its rows straight
 * into the all-to-all's send order (round 5, vdiff.dist.FrameShard.send_perm). */
int vd_gn_apply_rev3(const void* x0, int64_t ldx0, int64_t c0, const void* x1, int64_t ldx1,
                     int64_t C, int64_t n_inst, int64_t pix_per_inst, const float* scale_shift,
                     int32_t silu, void* y, int64_t ldy, int64_t n1, int64_t n2, int64_t inner,
                     vd_stream_t stream);
/* Two-launch GroupNorm for image instances (ResnetBlock2D / Transformer2DModel / VAE
 * norms): vd_gn_partial_g writes ONE {n, mean, M2} record per (instance, split, group)
 * (ws: n_inst*n_split*groups float4; C <= 2560, 256 % groups == 0), and vd_gn_apply_g
 * finalizes those records itself (prologue, per workgroup of rows_per_blk rows) before
 * applying y = (x-mean)*rstd*gamma + beta (+SiLU) — no finalize launch. */
int vd_gn_partial_g(const void* x0, int64_t ldx0, int64_t c0, const void* x1, int64_t ldx1,
                    int64_t C, int64_t n_inst, int64_t pix_per_inst, int32_t n_split,
                    int32_t groups, float* ws, vd_stream_t stream);
int vd_gn_apply_g(const void* x0, int64_t ldx0, int64_t c0, const void* x1, int64_t ldx1,
                  int64_t C, int64_t n_inst, int64_t pix_per_inst, const float* ws,
                  int32_t n_split_total, int32_t groups, float eps, const float* gamma,
                  const float* beta, int32_t silu, void* y, int64_t ldy, int64_t rows_per_blk,
                  vd_stream_t stream);
/* One-launch GroupNorm (+SiLU) for small image instances (round 5): one workgroup per (instance,
 * chunk of whole groups) holding its rows in registers, exact two-pass statistics, then the apply.
 * Taken when C / groups is a multiple of 8 and a chunk's rows fit 16 pieces of 8 channels per
 * thread (the UNet's levels 3-4 and mid block: pix <= 256); otherwise VD_EUNSUPPORTED, decided
 * from (pix_per_inst, C, groups) before any operand is read — callers may probe with null pointers
 * (vdiff.ops.gn_small_chunk mirrors the rule). */
int vd_gn_small(const void* x0, int64_t ldx0, int64_t c0, const void* x1, int64_t ldx1, int64_t C,
                int64_t n_inst, int64_t pix_per_inst, int32_t groups, float eps, const float* gamma,
                const float* beta, int32_t silu, void* y, int64_t ldy, vd_stream_t stream);
/* vd_gn_finalize over vd_gn_partial_g's per-group records (ws: n_inst*n_split_total*groups
 * float4, e.g. all-gathered from frame-sharded ranks) -> scale_shift[inst][C] {a, b}: the
 * motion-module norm, whose video instances need more records than vd_gn_apply_g's prologue
 * merges (round 5: C/groups times fewer records than vd_gn_partial's per-channel ones). */
int vd_gn_finalize_g(const float* ws, int64_t n_inst, int32_t n_split_total, int64_t C,
                     int32_t groups, float eps, const float* gamma, const float* beta,
                     float* scale_shift, vd_stream_t stream);
/* vd_gn_finalize_g over RANK-MAJOR records: ws = [n_ranks][n_inst][n_split_per_rank][groups]
 * float4, the frame-sharded ranks' all-gather output as it lands (round 6: no transpose copy into
 * vd_gn_finalize_g's [n_inst][n_ranks * n_split_per_rank][groups] order).  Split s of an instance
 * is rank s / n_split_per_rank's split s % n_split_per_rank, merged in vd_gn_finalize_g's order:
 * the result equals vd_gn_finalize_g on the transposed records bit for bit. */
int vd_gn_finalize_g_ranks(const float* ws, int64_t n_inst, int32_t n_ranks, int32_t n_split_per_rank,
                           int64_t C, int32_t groups, float eps, const float* gamma, const float* beta,
                           float* scale_shift, vd_stream_t stream);

/* ---------------------------------------------------------------- LayerNorm
 * BasicTransformerBlock.norm1/2/3 (eps 1e-5) over the last dim of bf16 rows,
 * optionally + pe[(row / pe_div) % pe_period][c] (fp32; the motion block's
 * SinusoidalPositionalEmbedding, applied after norm1 and norm2 — App. A.4).
 */
int vd_layernorm(const void* x, int64_t ldx, int64_t rows, int64_t C, const float* gamma,
                 const float* beta, float eps, const float* pe, int64_t pe_div,
                 int64_t pe_period, void* y, int64_t ldy, vd_stream_t stream);

/* ---------------------------------------------------------------- attention
 * softmax(q k^T * scale) v per (batch b, head h): replaces
 * F.scaled_dot_product_attention in Attention/AttnProcessor2_0 (a6 spatial
 * self-attention, a7 cross-attention).  Row (b, s) of q at q + (b*sq + s)*ldq,
 * head h at column h*d.  K/V batch index = b / kv_div (cross-attention reads the
 * un-repeated encoder_hidden_states projection once per video).
 * d in {32, 40, 64, 80, 128, 160, 512}; flash (online softmax) with bf16 MFMA.  d = 512
 * (round 3) is the VAE decoder's single-head mid-block Attention (diffusers AttnProcessor2_0
 * over the 64x64 latent pixels of each frame): flash512_kernel,
 * o 16-byte aligned with ldo % 8 == 0 (bf16) / % 4 == 0 (fp32).
 */
int vd_attention(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                 int64_t ldv, void* o, int64_t ldo, int64_t batch, int32_t heads, int64_t sq,
                 int64_t skv, int32_t d, int64_t kv_div, float scale, vd_stream_t stream);
/* vd_attention with the output O in fp32 (o: float rows, ldo in floats, 16-byte aligned):
 * the same kernels and arithmetic, minus the final bf16 rounding of O — the parity tests
 * hold it to rtol 1e-3 / atol 1e-4 against an fp64 reference. */
int vd_attention_f32(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                     int64_t ldv, float* o, int64_t ldo, int64_t batch, int32_t heads,
                     int64_t sq, int64_t skv, int32_t d, int64_t kv_div, float scale, vd_stream_t stream);
/* vd_attention / vd_attention_f32 with an explicit kernel choice per call (the library keeps no
 * selector state): kernel 0 = the automatic choice (what vd_attention runs: d = 40 -> flash40
 * from 4 key tiles, flash32 below; d = 80 -> flash80 from 4 key tiles (round 6); other d -> the
 * 16x16x32 flash kernel), 1 = the 16x16x32 flash kernel for any d, 2 = flash32 (d = 40),
 * 3 = flash40 / flash80 wherever they apply (d = 40 / 80, >= 2 key tiles); a kernel that does not
 * take the shape falls through to the next one down (vd_attention_plan names the one that runs).  All of
 * them compute softmax(q k^T * scale) v; flash40 is bit-identical to flash32 (the parity tests
 * run each).  out_f32 as vd_attention_f32.
 * VD_ATTN_CAUSAL OR-ed into kernel: query i attends to keys j <= i only (the CLIP text encoder's
 * self-attention).  It needs sq == skv and kv_div == 1 (else VD_EINVAL), scale > 0 (else
 * VD_EINVAL) and d in {32, 64} (else VD_EUNSUPPORTED); it always runs the 16x16x32 flash kernel,
 * whose causal instances skip the key tiles wholly above the diagonal.  Any other bit above the
 * low byte is VD_EINVAL.  vd_attention and vd_attention_f32 are never causal.
 * VD_ATTN_TAIL(n) OR-ed into kernel, 1 <= n <= 64: two-segment attention (the IP-Adapter image
 * prompt).  Of the skv K/V rows of a key batch, rows [0, skv - n) are segment A (the text) and rows
 * [skv - n, skv) are segment B (the image tokens); each segment has a softmax of its own and
 *     o = softmax(q K_A^T scale) V_A + softmax(q K_B^T scale) V_B,
 * summed in fp32 before the one store (an adapter scale is folded into V_B by the caller).
 * kv_div, the row strides, out_f32 and the batch layout (k + bkv*skv*ldk) are those of an
 * untailed call.  It needs n < skv, no VD_ATTN_CAUSAL and scale > 0 (else VD_EINVAL; n > 64 does
 * not fit the mask) and d in {32, 40, 64, 80, 160} (else VD_EUNSUPPORTED); it always runs the
 * 16x16x32 flash kernel whatever the low byte says.  With V_B = 0 the result is bit-identical to
 * kernel = 1 on segment A alone.  vd_attention and vd_attention_f32 never take a tail. */
enum { VD_ATTN_CAUSAL = 0x100 };
enum { VD_ATTN_TAIL_SHIFT = 16, VD_ATTN_TAIL_MASK = 0x7f0000 };
#define VD_ATTN_TAIL(n) ((n) << VD_ATTN_TAIL_SHIFT)
int vd_attention_ex(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                    void* o, int64_t ldo, int64_t batch, int32_t heads, int64_t sq, int64_t skv, int32_t d,
                    int64_t kv_div, float scale, int32_t out_f32, int32_t kernel, vd_stream_t stream);
/* The plan vd_attention_ex would run for these sizes, this output address (read as a number,
 * never dereferenced) and stride, and this kernel word (VD_ATTN_CAUSAL / VD_ATTN_TAIL included):
 * host only, no launch, no device needed.  Returns what the call would return before it
 * launches, as far as it depends on these arguments (the q / k / v pointers and strides are
 * not asked about): VD_OK, VD_EINVAL or VD_EUNSUPPORTED, with every output 0 unless VD_OK.
 *   *family      the kernel family, VD_ATTN_K_* — where a forced kernel did not take the shape,
 *                the one it fell through to
 *   *qblk        VD_ATTN_K_FLASH: 16-query blocks per wave, 2 or 4 (a workgroup holds 64 * qblk
 *                queries); 0 for the other families
 *   *unit_scale  flash32 / flash40 / flash80: 1 when scale * log2(e) == 1 in fp32 and the
 *                instance without the per-score multiply runs; 0 for the other families
 *   *grid        workgroups of the (first) launch
 *   *exact_grid  VD_ATTN_K_FLASH40: workgroups of flash32's exact pass launched after it (16 of its
 *                128-query blocks each; a block reruns when flash40 left a NaN flag in the block's
 *                own first output element, one flag per 128 queries); else 0 */
enum {
  VD_ATTN_K_FLASH = 1,    /* the 16x16x32 flash kernel (plain, causal, tailed) */
  VD_ATTN_K_FLASH32 = 2,  /* d = 40 */
  VD_ATTN_K_FLASH40 = 3,  /* d = 40, >= 2 key tiles */
  VD_ATTN_K_FLASH80 = 4,  /* d = 80, >= 2 key tiles */
  VD_ATTN_K_FLASH512 = 5  /* d = 512 */
};
int vd_attention_plan(const void* o, int64_t ldo, int64_t batch, int32_t heads, int64_t sq, int64_t skv, int32_t d,
                      int64_t kv_div, float scale, int32_t out_f32, int32_t kernel, int32_t* family, int32_t* qblk,
                      int32_t* unit_scale, int64_t* grid, int64_t* exact_grid);

/* Temporal (motion-module) self-attention over frames (a9): token (b, f, p) is
 * row (b*frames + f)*positions + p of q/k/v/o (the NHWC layout, no permute);
 * frames <= 32. */
int vd_temporal_attention(const void* q, const void* k, const void* v, int64_t ld,
                          void* o, int64_t ldo, int64_t batch, int32_t frames,
                          int64_t positions, int32_t heads, int32_t d, float scale,
                          vd_stream_t stream);
/* Temporal attention of a frame-sharded rank under the K/V all-gather layout (SURVEY.md §8e,
 * the north star's "RCCL all-gather for the temporal-attention window"): the rank's own
 * qframes query frames, rows (b*qframes + f)*positions + p of q (stride ldq) and o (stride
 * ldo), against all kframes key frames gathered from every rank, rows
 * (b*kframes + f)*positions + p of k and v (stride ldkv).  Replaces, for the rank's frames,
 * the rows of diffusers' temporal Attention (motion_module.py: attention over the
 * (B*H*W, F, C) sequence; 03_trace_forward_pass.py:160-169).  qframes <= kframes <= 16;
 * d in {32, 40, 64, 80, 160} (else VD_EUNSUPPORTED). */
int vd_temporal_attention_kv(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                             void* o, int64_t ldo, int64_t batch, int32_t qframes, int32_t kframes,
                             int64_t positions, int32_t heads, int32_t d, float scale,
                             vd_stream_t stream);
/* The motion module's temporal self-attention WITH its Q/K/V projection (round 2): x = the
 * normed rows (b, f, p) [row stride ldx] of one BasicTransformerBlock attention
 * (AnimateDiffTransformer3D, a8/a9), wqkv = the fused [3C][C] to_q|to_k|to_v weight (the
 * softmax scale folded into to_q as vdiff's Attention.prepare does, or passed as `scale`),
 * o = the attention output rows [row stride ldo], before to_out.  Equal bit for bit to
 * vd_gemm(x, wqkv) followed by vd_temporal_attention; the [rows][3C] projection never
 * reaches HBM.  Implemented for the level-1 shape (frames 16, 8 heads, d 40) with at least
 * two workgroups (8 positions of one video each) per CU; else VD_EUNSUPPORTED — callers run
 * the two-launch path. */
int vd_motion_qkv_attention(const void* x, int64_t ldx, const void* wqkv, int64_t ldw, void* o, int64_t ldo,
                            int64_t batch, int32_t frames, int64_t positions, int32_t heads, int32_t d,
                            float scale, const float* ln_fold_tab, float ln_fold_eps, vd_stream_t stream);
/* ln_fold_tab != NULL (round 5): the block's LayerNorm (+ the sinusoidal PE by frame) folded in,
 * as vd_gemm_desc.ln_fold_s: x holds the UN-normalised rows, wqkv = W_qkv∘gamma (bf16), and
 * ln_fold_tab is [8 heads][2048] fp32: per head h, the 120 row sums of wqkv's rows of that head
 * (q | k | v, 40 each, in that order), then for each frame f < 16 the 120 values
 * W·(beta + pe[f]) of the same rows (W the unfolded fp32 weight), zero-padded to 2048.
 * vd_motion_qkv_attention_takes: 1 when the fused kernel takes the shape (else the call
 * returns VD_EUNSUPPORTED and the caller runs GEMM + vd_temporal_attention); no launch. */
int vd_motion_qkv_attention_takes(int64_t batch, int32_t frames, int64_t positions, int32_t heads, int32_t d);
/* vd_temporal_attention for the DiT's temporal blocks (d = 64, 17..32 frames) with the 1-D
 * temporal RoPE (vd_rope_qk mode 1, angle by frame) applied to q/k inside the kernel as they
 * are loaded; q and k are read un-rotated and left unchanged. */
int vd_temporal_attention_rope(const void* q, const void* k, const void* v, int64_t ld, void* o,
                               int64_t ldo, int64_t batch, int32_t frames, int64_t positions,
                               int32_t heads, int32_t d, float scale, float theta,
                               vd_stream_t stream);
/* vd_temporal_attention on the VALU kernel for every shape (vd_temporal_attention takes the
 * MFMA kernel for frames <= 16 and d in {32, 40, 64, 80, 160}, frames 17..32 and d in {40, 64, 80,
 * 160}, and this one otherwise): the same arguments and result; the parity tests run both. */
int vd_temporal_attention_valu(const void* q, const void* k, const void* v, int64_t ld, void* o,
                               int64_t ldo, int64_t batch, int32_t frames, int64_t positions,
                               int32_t heads, int32_t d, float scale, vd_stream_t stream);

/* Row softmax over fp32 scores in log2 units (p = exp2(s - max) / sum, bf16 out): round 2's
 * materialised-score form of the VAE mid-block attention (now vd_attention with d = 512;
 * kept for tools/vae_attn_ab.py's A/B and as a general row softmax).
 * rows x cols, cols % 4 == 0, row strides ld_s / ld_p in elements. */
int vd_softmax_rows(const float* s, int64_t ld_s, int64_t rows, int64_t cols, void* p,
                    int64_t ld_p, vd_stream_t stream);

/* Temporal-consistency metric cores (experiments/
 * 06_measure_grid_search.py compute_mse :209-211 over consecutive frames and
 * compute_flicker_index :221-235) for a batch of uint8 videos [videos][frames][bytes]
 * (bytes_per_frame = H*W*3, multiple of 16, base 16-byte aligned), exact integers:
 *   sse[v][f] = sum (x[f+1]-x[f])^2 (f < frames-1); sad[v][f] = sum |x[f]-2x[f+1]+x[f+2]|
 * (f < frames-2; sad may be NULL when frames == 2).  2 <= frames <= 32. */
int vd_frame_metrics(const void* frames_u8, int64_t videos, int32_t frames, int64_t bytes_per_frame,
                     uint64_t* sse, uint64_t* sad, vd_stream_t stream);

/* Dense optical flow of every consecutive frame pair (replaces
 * OpticalFlowEstimator.compute_flow, experiments/06_measure_grid_search.py:163-188 =
 * cv2.calcOpticalFlowFarneback(grey_f, grey_f+1, None, pyr_scale, levels, winsize,
 * iterations, poly_n, poly_sigma, flags=0) with grey = uint8(mean_c(x/255)*255), :173).
 * frames_u8: [videos][frames][H][W][3] uint8; flow out: fp32 [videos][frames-1][H][W][2]
 * (dx, dy); poly_n 5 or 7; workspace: at least the byte count vd_farneback_workspace
 * returns for the same sizes (-1 on bad sizes), device memory. */
int64_t vd_farneback_workspace(int64_t videos, int32_t frames, int32_t H, int32_t W);
int vd_farneback_flow(const void* frames_u8, int64_t videos, int32_t frames, int32_t H, int32_t W,
                      double pyr_scale, int32_t levels, int32_t winsize, int32_t iterations,
                      int32_t poly_n, double poly_sigma, float* flow, void* workspace,
                      int64_t workspace_bytes, vd_stream_t stream);

/* Flow magnitude moments and warp error per pair (06:190-199 compute_flow_stats,
 * :259-284 warp_frame, :336-337): stats [videos*(frames-1)][3] fp64 =
 * { sum |flow|, sum |flow|^2 over H*W, sum over 3*H*W of (warp(frame_f, flow) - frame_f+1)^2 }
 * with frames as u8/255, warp = grid_sample(bilinear, border, align_corners=True) at
 * (x + dx, y + dy).  Deterministic (fixed-order partials in the workspace: at least the
 * byte count vd_flow_warp_workspace returns). */
int64_t vd_flow_warp_workspace(int64_t videos, int32_t frames);
int vd_flow_warp_stats(const void* frames_u8, const float* flow, int64_t videos, int32_t frames,
                       int32_t H, int32_t W, double* stats, void* workspace, int64_t workspace_bytes,
                       vd_stream_t stream);

/* LPIPS over consecutive frames (experiments/06_measure_grid_search.py:122-154 LPIPSMetric =
 * lpips.LPIPS(net='alex', version='0.1'), eval mode), exact fp32: every convolution runs on
 * the f32-input MFMA (v_mfma_f32_16x16x4_f32, bit-for-bit a k-ordered fmaf chain), no split-K
 * and no float atomics, so results are deterministic and an image's value does not depend on
 * the rest of the batch.
 *
 * vd_conv2d_f32: y = [relu](conv2d(x, w) + bias), NHWC fp32.  x [N][H][W][Cin], w
 *   [Cout][kh][kw][Cin], bias [Cout] or NULL, y [N][OH][OW][Cout] with OH = (H + 2 pad - kh) /
 *   stride + 1 (OW alike), zero padding.  Cout % 64 == 0; Cin % 4 == 0 (x and w 16-byte aligned)
 *   or Cin == 3; x and y below 2^31 elements.
 * vd_lpips_layer: one tap's distance for `pairs` pairs of feature maps fa, fb [pairs][pixels][C]
 *   fp32: n = f / (sqrt(sum_c f^2) + 1e-10) per pixel, d = mean over pixels of
 *   sum_c lin[c] (n_a - n_b)^2; out[p] = d if !accumulate, out[p] += d otherwise (fp64).
 *   C % 64 == 0, C <= 512; per-pixel sums fp32, across pixels fp64 in a fixed order through the
 *   workspace (at least the byte count vd_lpips_layer_workspace returns for `pairs`; -1 on
 *   pairs < 1).
 * vd_lpips_pairs: frames_u8 [videos][frames][H][W][3] uint8 -> out [videos][frames-1] fp64 =
 *   LPIPS(frame f, frame f+1).  Per image: x = 2 u / 255 - 1, (x - shift) / scale, the five
 *   ReLU taps of AlexNet `features` (conv(3,64,11,s4,p2); pool; conv(64,192,5,p2); pool;
 *   conv(192,384,3,p1); conv(384,256,3,p1); conv(256,256,3,p1); pool = MaxPool2d(3, 2)), computed
 *   once per frame; per pair the sum of the five vd_lpips_layer distances.  H, W >= 31, frames
 *   >= 2.  params: one fp32 blob, 16-byte aligned, 2,470,854 floats in this order:
 *     conv weights 1..5, each [Cout][k][k][Cin]   at float offset 0, 23232, 330432, 993984, 1878720
 *     conv biases 1..5  (64,192,384,256,256)      at 2468544, 2468608, 2468800, 2469184, 2469440
 *     lin vectors 1..5  (64,192,384,256,256)      at 2469696, 2469760, 2469952, 2470336, 2470592
 *     shift[3], scale[3]                           at 2470848, 2470851
 *   workspace: at least the byte count vd_lpips_workspace returns for images = videos * frames,
 *   device memory, 16-byte aligned (-1 on H or W < 31 or a batch whose buffers pass 2^31
 *   elements). */
int vd_conv2d_f32(const float* x, int64_t N, int32_t H, int32_t W, int32_t Cin, const float* w,
                  const float* bias, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                  int32_t pad, int32_t relu, float* y, vd_stream_t stream);
int64_t vd_lpips_layer_workspace(int64_t pairs);
int vd_lpips_layer(const float* fa, const float* fb, int64_t pairs, int64_t pixels, int32_t C,
                   const float* lin, double* out, int32_t accumulate, void* workspace,
                   int64_t workspace_bytes, vd_stream_t stream);
int64_t vd_lpips_workspace(int64_t images, int32_t H, int32_t W);
int vd_lpips_pairs(const void* frames_u8, int64_t videos, int32_t frames, int32_t H, int32_t W,
                   const float* params, double* out, void* workspace, int64_t workspace_bytes,
                   vd_stream_t stream);

/* ---------------------------------------------------------------- step glue
 * vd_timestep_embed: diffusers Timesteps(dim, flip_sin_to_cos=True, shift 0)
 *   (a12) -> bf16 [B][dim].  Timestep = ts[*step_idx] if step_idx else ts[b]; ts holds
 *   n_ts entries (the device step index is clamped to [0, n_ts - 1]; without step_idx
 *   n_ts >= B).
 * vd_pack_latents: x (B,C,F,H,W) fp32 / in_div -> NHWC bf16 rows [(dup*B*F*H*W)][cpad],
 *   channels >= C zero; dup = 2 repeats the batch (the CFG cat([x, x])); in_div is
 *   the scheduler's scale_model_input divisor (1 for DDIM, sqrt(sigma^2+1) for Euler).
 * vd_unpack_nhwc: NHWC rows (fp32 if src_f32 else bf16, row stride ld) ->
 *   (B,C,F,H,W) fp32.
 * vd_ddim_cfg_step: eps rows NHWC fp32 [(ncfg*B*F*H*W)][ld_eps]; if ncfg == 2
 *   eps = e_u + g*(e_c - e_u) (uncond first); DDIM eta=0 epsilon update of
 *   latents (B,C,F,H,W) fp32 in place with coef[4*step] = {sqrt(a_t),
 *   sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)}, step = *step_idx (or 0 if
 *   NULL) clamped to the n_coef rows of the table; fp32 in diffusers' operation
 *   order, one rounding per op (bit-exact vs torch); optional x0_out (B,C,F,H,W) fp32; optional next_in = the packed
 *   bf16 UNet input of the next step (dup = ncfg) — a1 + a13 fused.  next_in is written whole, as
 *   vd_pack_latents writes it: ncfg * B*F*H*W contiguous rows of cpad channels, the padding
 *   [C, cpad) zero — it need not have been packed (or initialised) before.
 * vd_euler_cfg_step: as vd_ddim_cfg_step, with the EulerDiscreteScheduler.step
 *   update (s_churn 0, epsilon; diffusers' fp32 order x0 = x - s*eps,
 *   d = (x - x0)/s, x += d*(s_next - s)) and coef[4*step] = {sigma, sigma_next,
 *   sqrt(sigma_next^2 + 1), 0}; next_in = the next step's scale_model_input(x)
 *   packed to bf16 — §8f rank 2 (experiments/01_baseline_generation.py:76-80).
 *   It refuses VD_STEP_LCM (VD_EINVAL).
 * VD_STEP_LCM OR-ed into vd_ddim_cfg_step's ncfg (the low byte stays 1 or 2; any other bit above
 *   it is VD_EINVAL): the diffusers LCMScheduler.step update (epsilon prediction) instead of DDIM's,
 *     x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t);  den = c_out*x0 + c_skip*x
 *     x <- add_noise ? sqrt(a_prev)*den + sqrt(1-a_prev)*noise : den
 *   with the same one-rounding-per-op fp32 arithmetic; x0_out receives den (diffusers' `denoised`),
 *   next_in bf16(x) as above.  It rides on this entry point instead of a new symbol, as
 *   VD_CONV_PAD_END and VD_ATTN_TAIL ride on theirs, and the signature has no spare pointer, so
 *   the per-step noise travels in coef: one fp32 buffer, 16-byte aligned, of
 *     n_coef rows of 8 floats {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev), c_skip,
 *       c_out, add_noise (0.0 or 1.0), 0}, then
 *     n_coef slabs of B*C*F*H*W floats in (B,C,F,H,W) order, from float offset 8*n_coef.
 *   Step st (= *step_idx clamped to the n_coef rows) reads row st and, only when that row's
 *   add_noise != 0, slab st: the last step's slab is sized but never read.  Step index, branch
 *   and noise are all read inside the launch, so a captured step replays over the whole schedule.
 * VD_STEP_DPM OR-ed into vd_ddim_cfg_step's ncfg (0x400: 0x200 stays VD_EINVAL; together with
 *   VD_STEP_LCM it is VD_EINVAL; vd_euler_cfg_step refuses it): the diffusers
 *   DPMSolverMultistepScheduler.step update — "dpmsolver++" and "sde-dpmsolver++", midpoint,
 *   solver order 1 or 2, epsilon prediction — in the same one-rounding-per-op fp32 arithmetic:
 *     x0 = (x - sigma_s*eps) / alpha_s
 *     x  <- c_x*x + c_m0*x0
 *     second order:  x <- x + c_d1 * ((1/r0) * (x0 - m1))
 *     SDE noise:     x <- x + c_noise * noise
 *   coef is 16-byte aligned and holds n_coef rows of 8 floats
 *     {alpha_s, sigma_s, c_x, c_m0, c_d1, 1/r0, c_noise, flags}, flags = 1.0 * second order +
 *     2.0 * SDE noise; a slot its row does not use holds 0.0 and the whole table is finite.
 *   diffusers writes the deterministic update with two subtractions; the host stores those two
 *   coefficients (c_m0, c_d1) negated, so one add-only form serves both algorithm types
 *   (a - c*b == a + (-c)*b bit for bit).  When any row has the SDE flag, n_coef slabs of
 *   B*C*F*H*W floats follow from float offset 8*n_coef, as under VD_STEP_LCM; an SDE row reads
 *   its slab on every step, the last included (its c_noise is 0 there, the slab must be finite).
 *   x0_out is REQUIRED and is both input and output, the multistep history: on entry the previous
 *   step's x0 (m1), read only when the row's second-order flag is set; on exit this step's x0.
 *   Each thread reads m1[i] before it writes x0[i].  x0_out == NULL or x0_out == latents is
 *   VD_EINVAL.  A first-order row (step 0 of any schedule) never reads it, so the history needs
 *   no clearing between schedules.
 * VD_STEP_UNIPC OR-ed into vd_ddim_cfg_step's ncfg (0x2000: 0x200 and 0x1000 stay VD_EINVAL;
 *   together with VD_STEP_LCM or VD_STEP_DPM it is VD_EINVAL; vd_euler_cfg_step refuses it; with
 *   VD_STEP_PAG it combines as VD_STEP_DPM does, the PAG scales in front of the rows): the
 *   diffusers UniPCMultistepScheduler.step update — predict_x0, solver_type "bh1" or "bh2", solver
 *   order 1 or 2, epsilon prediction — the corrector of the previous step and the predictor of
 *   this one in one pass, in the same one-rounding-per-op fp32 arithmetic, in exactly this order:
 *     m_t = (x - sigma_s*eps) / alpha_s
 *     xc  = x
 *     flags & 1 (the corrector runs):
 *       x_  = c_last*S2 - c_m*S0
 *       d_t = m_t - S0
 *       r   = flags & 2 ? rho0*((S1 - S0) / rk_c) + rhot*d_t : rhot*d_t
 *       xc  = x_ - c_B*r
 *     y = p_x*xc - p_m*m_t
 *     flags & 4 (a second-order predictor):  y = y - p_B*(0.5*((S0 - m_t) / rk_p))
 *     latents <- y;  S1 <- S0;  S0 <- m_t;  S2 <- xc;  next_in <- bf16(y) per branch
 *   both divisions correctly rounded.  coef is 16-byte aligned and holds n_coef rows of 16 floats
 *     {alpha_s, sigma_s, c_last, c_m, c_B, rk_c, rho0, rhot, p_x, p_m, p_B, rk_p, flags, 0, 0, 0}
 *     c_last = sig_i/sig_{i-1}, c_m = alpha_i*h_phi_1 and c_B = alpha_i*B_h of the corrector's
 *     step i-1 -> i; p_x = sig_{i+1}/sig_i, p_m = alpha_{i+1}*h_phi_1 and p_B = alpha_{i+1}*B_h of
 *     the predictor's step i -> i+1; rk_c, rk_p the ratios of the log-SNR steps (negative);
 *     (rho0, rhot) the corrector's weights, (0, 0.5) at first order; flags = 1.0 * the corrector
 *     runs + 2.0 * it is second order + 4.0 * the predictor is second order.  A slot its row does
 *     not use holds 0.0 and is never read — the kernel never divides by an unused rk — and the
 *     whole table is finite (a final sigma of 0 gives p_x = 0, p_m = -1: y = m_t).
 *   x0_out is REQUIRED and is both input and output, the solver's state: THREE contiguous slabs of
 *   N = B*C*F*H*W floats, S0 the latest x0 prediction, S1 the one before it, S2 `last`, the sample
 *   the previous predictor started from.  Each thread reads its element of every slab the row
 *   needs before it writes any, and all three slabs are written on every step.  A row with
 *   flags 0 (step 0 of any run) reads no slab and starts the history (S1 <- m_t as well); only a
 *   second-order corrector reads S1; so the state needs no clearing between schedules.
 *   x0_out == NULL, or [x0_out, x0_out + 3N) overlapping [latents, latents + N), is VD_EINVAL.
 * VD_STEP_ANCESTRAL OR-ed into vd_euler_cfg_step's ncfg (0x4000: 0x200 and 0x1000 stay VD_EINVAL;
 *   together with VD_STEP_LCM, VD_STEP_DPM or VD_STEP_UNIPC it is VD_EINVAL; vd_ddim_cfg_step
 *   refuses it, as any bit it does not know; with VD_STEP_PAG it combines exactly as plain Euler
 *   does, the PAG scales in front of the rows and the low byte 2 or 3): the diffusers
 *   EulerAncestralDiscreteScheduler.step update (epsilon prediction) instead of Euler's, after the
 *   unchanged guidance / PAG combine, in the same one-rounding-per-op fp32 arithmetic, in exactly
 *   this order:
 *     x0 = x - sigma*eps
 *     d  = (x - x0) / sigma
 *     x  <- x + d*(sigma_down - sigma)
 *     x  <- x + noise*sigma_up                       (only if sigma_up != 0)
 *     next_in <- bf16(x / sqrt(sigma_to^2 + 1)) per branch, the padding columns zero
 *   both divisions correctly rounded; x0_out is optional and receives x0, as without the flag.
 *   It rides on this entry point instead of a new symbol, as VD_STEP_LCM rides on
 *   vd_ddim_cfg_step, and the per-step noise travels in coef the same way: one fp32 buffer,
 *   16-byte aligned (else VD_EINVAL), of
 *     n_coef rows of 4 floats {sigma, sigma_down, sqrt(sigma_to^2 + 1), sigma_up} — Euler's row
 *       with sigma_next replaced by sigma_down and its unused zero by sigma_up (sigma_to is the
 *       schedule's next sigma; sigma_up^2 + sigma_down^2 = sigma_to^2), then
 *     n_coef slabs of B*C*F*H*W floats in (B,C,F,H,W) order, from float offset 4*n_coef.
 *   Step st (= *step_idx clamped to the n_coef rows) reads row st and, only when that row's
 *   sigma_up != 0, slab st: the last step of every schedule has sigma_to = 0, hence sigma_up =
 *   sigma_down = 0, so its slab is sized but never read, and whatever it holds, NaN included,
 *   reaches no output.  A plain Euler table (sigma_down = sigma_next, slot 3 = 0) under the flag
 *   therefore gives the unflagged kernel's result bit for bit.  Step index, row and noise are all
 *   read inside the launch, so a captured step replays over the whole schedule.  This library
 *   cannot check the buffer's size; the caller does (vdiff.ops.euler_ancestral_cfg_step).
 * VD_STEP_PAG OR-ed into ncfg (0x800) of vd_ddim_cfg_step — alone, or with VD_STEP_LCM,
 *   VD_STEP_DPM or VD_STEP_UNIPC — or of vd_euler_cfg_step, alone or with VD_STEP_ANCESTRAL:
 *   perturbed-attention guidance (diffusers' PAGMixin).  The
 *   low byte is then 2 or 3 (anything else is VD_EINVAL; without the flag 3 stays VD_EINVAL):
 *     3: eps rows [uncond; cond; perturbed], each of B*F*H*W rows,
 *          e = (e_u + g*(e_c - e_u)) + s*(e_c - e_p)
 *     2: eps rows [cond; perturbed] (no CFG; guidance is ignored),
 *          e = e_c + s*(e_c - e_p)
 *   in the same one-rounding-per-op fp32 arithmetic, in exactly this order; the scheduler update
 *   that follows is unchanged.  s is the per-step PAG scale (it changes with the step under
 *   adaptive scaling) and travels in coef, which under the flag must be 16-byte aligned and holds
 *     n_coef fp32 PAG scales, padded with (-n_coef mod 4) floats to a multiple of 4 (the padding
 *       is never read), then
 *     the scheduler's unchanged layout, from float offset 4*ceil(n_coef/4): n_coef rows of 4
 *       (DDIM, Euler, Euler ancestral), 8 (LCM, DPM) or 16 (UniPC) floats and, where that scheduler
 *       has them, its n_coef noise slabs behind the rows.  The padding keeps the 16-byte alignment
 *       LCM, DPM, UniPC and Euler ancestral ask for.
 *   s = pag[st], st the same clamped device step index that picks the coefficient row, read inside
 *   the launch.  The scales must be finite and >= 0; this library cannot read device memory, so
 *   the caller checks that (vdiff.ops.pag_coef does).  next_in receives one copy of the packed
 *   input per branch (2 or 3), the padding columns of every copy zero.  x0_out, DPM's history and
 *   LCM's `denoised` keep their meaning.
 * vd_step_advance: ++*step_idx (one thread; the last node of a captured step).
 */
enum { VD_STEP_LCM = 0x100 }; /* OR-ed into vd_ddim_cfg_step's ncfg, see above */
enum { VD_STEP_DPM = 0x400 }; /* likewise; x0_out becomes the in/out history, see above */
enum { VD_STEP_PAG = 0x800 }; /* into either step's ncfg: a third branch, scales in front of coef */
enum { VD_STEP_UNIPC = 0x2000 }; /* as VD_STEP_DPM; x0_out becomes the in/out three-slab state, see above */
enum { VD_STEP_ANCESTRAL = 0x4000 }; /* into vd_euler_cfg_step's ncfg: the stochastic step, noise slabs behind the rows */
int vd_timestep_embed(const float* ts, int64_t n_ts, const int32_t* step_idx, int64_t B,
                      int32_t dim, void* out, vd_stream_t stream);
int vd_pack_latents(const float* x, int64_t B, int64_t C, int64_t F, int64_t H, int64_t W,
                    int32_t dup, void* out, int64_t cpad, float in_div, vd_stream_t stream);
int vd_unpack_nhwc(const void* src, int32_t src_f32, int64_t ld, int64_t B, int64_t C,
                   int64_t F, int64_t H, int64_t W, float* dst, vd_stream_t stream);
int vd_ddim_cfg_step(const float* eps, int64_t ld_eps, int32_t ncfg, float guidance,
                     float* latents, int64_t B, int64_t C, int64_t F, int64_t H, int64_t W,
                     const float* coef, int64_t n_coef, const int32_t* step_idx, float* x0_out,
                     void* next_in, int64_t cpad, vd_stream_t stream);
int vd_euler_cfg_step(const float* eps, int64_t ld_eps, int32_t ncfg, float guidance,
                      float* latents, int64_t B, int64_t C, int64_t F, int64_t H, int64_t W,
                      const float* coef, int64_t n_coef, const int32_t* step_idx, float* x0_out,
                      void* next_in, int64_t cpad, vd_stream_t stream);
int vd_step_advance(int32_t* step_idx, vd_stream_t stream);

/* Row-block permute for the frame<->position re-shard around motion modules:
 * dst[(a*nb + b)*nc + c] = src[(b*na + a)*nc + c] for bf16 rows of `width`
 * elements (a transpose of the [nb][na] grid of row blocks, nc rows each). */
int vd_block_transpose(const void* src, void* dst, int64_t nb, int64_t na, int64_t nc,
                       int64_t width, vd_stream_t stream);

/* ---- module-level (diffusers-layout) path: csrc/rows.hip ----
 * Elementwise ops a caller driving the modules one by one needs between HIP GEMM / norm /
 * attention calls (forward-hook tracing, experiments/03_trace_forward_pass.py:105-113; a
 * direct motion_modules[i](x, num_frames=F) call, 03:182).  bf16 rows, C % 8 == 0, 16-B
 * aligned bases, row strides in elements.
 * vd_rows_eltwise: op 0: out[r] = (x ? x[r] : 0) + y[(r / y_div) % y_period] (y bf16, or fp32
 *   if y_f32) — residual adds, the ResnetBlock2D time-embedding broadcast, the sinusoidal
 *   positional embedding, repeat_interleave, channel concat into column slices;
 *   op 1: out[r] = silu(x[r]) (nn.SiLU).
 *   Ops 2 and 3 are FreeU (diffusers' apply_freeu, run before each skip concat of up_blocks[0]
 *   and [1]).  They ride on this entry point instead of a new symbol, as VD_CONV_PAD_END and
 *   VD_ATTN_TAIL ride on theirs: the operands are the same bf16 rows with the same alignment
 *   rules, and the set of exported symbols (vd_version 6) stays what it is.  The signature has
 *   no float slot, so both read their scalar from DEVICE memory, inside the launch only (the
 *   call stays graph-capturable and the value may change between replays): y points to one
 *   fp32, 4-byte aligned, with y_f32 == 1 and ldy == 0 (anything else is VD_EINVAL).
 *   op 2, VD_ROWS_FREEU_FILTER: diffusers' fourier_filter(x, threshold=1, scale=*y) on the rows
 *   of n_img H x W images, H = y_period, W = y_div, rows = n_img * H * W.  threshold 1 scales
 *   the four frequency bins k_h, k_w in {-1, 0} only, so per (image, channel) plane, with
 *   th = 2 pi h / H and tw = 2 pi w / W,
 *     out = x + (s - 1) / (H W) * (A + B cos th + C sin th + D cos tw + E sin tw
 *                                    + P cos(th + tw) + Q sin(th + tw)),
 *   A .. Q the plane's sums of x times the same seven factors.  One launch; fp32 sums in an
 *   order fixed by (H, W) alone (never by n_img, the image's index or C: a frame-sharded call
 *   matches the unsharded one bit for bit), no atomics; one rounding to bf16, of
 *   fmaf((s - 1) / (H W), corr, x), so s == 1 returns x (a -0 may come back as +0: 0 * corr is
 *   added to it).  out may be a column slice of a wider
 *   buffer.  VD_EINVAL: H < 2 or W < 2 (the 2 x 2 box collapses), H + W > 4096, rows not a
 *   multiple of H * W, x or y NULL, out == x.
 *   op 3, VD_ROWS_SCALE: out[r][c] = bf16(x[r][c] * *y) over C columns; out == x is allowed
 *   (FreeU's hidden_states[:, :C/2] *= b, on the column slice alone).  y_div and y_period are
 *   not read.
 *   Ops 4 and 5 are FreeNoise (diffusers' FreeNoiseTransformerBlock: a motion transformer block
 *   runs on sliding windows of L frames and the window outputs are averaged with per-frame
 *   weights).  They ride on this entry point for the same reason as ops 2 and 3.  The rows are
 *   (video b, frame f, position p); op = VD_ROWS_WIN_GATHER or VD_ROWS_WIN_MERGE, OR-ed with
 *   VD_ROWS_WIN_STRIDE(s) (the low byte is the op, as VD_ATTN_TAIL(n) rides on its kernel word);
 *   F = y_period frames, hw = y_div positions per frame, L = ldy the context length, rows =
 *   B * F * hw the UN-windowed row count.  Windows, with integer division: nReg = (F - L) / s + 1
 *   regular windows start at frame w * s; when (nReg - 1) * s + L < F one more tail window starts
 *   at F - L and owns the last tail_len = F - ((nReg - 1) * s + L) frames; nW = nReg (+ 1).
 *   op 4, VD_ROWS_WIN_GATHER: out[((b * nW + w) * L + j) * hw + p] = x[(b * F + start_w + j) * hw + p],
 *   a 16-byte copy: the rows of B * nW videos of L frames, which the temporal kernels take as
 *   they are.  x holds rows rows, out B * nW * L * hw.  y == NULL and y_f32 == 0.
 *   op 5, VD_ROWS_WIN_MERGE, the inverse: x holds the B * nW * L * hw window rows, out rows rows.
 *   A frame f that regular windows cover becomes
 *     out = bf16( (sum_w wt[f - w s] * x_w[f - w s]) / (sum_w wt[f - w s]) ),
 *   both sums in fp32 over the regular windows that hold f in ascending w (fmaf per term, one
 *   correctly rounded division, one rounding to bf16; no atomics), so the order depends on
 *   (F, L, s) alone, never on B, hw or C.  The last tail_len frames, which no regular window
 *   reaches, take the tail window's value as it is; the tail window's other frames are not read.
 *   y = L fp32 weights in DEVICE memory (y_f32 == 1, 4-byte aligned), read inside the launch
 *   only, so the call stays graph-capturable.  They must be finite and positive: that is the
 *   caller's duty, the entry point cannot refuse a device value.
 *   VD_EINVAL for both: s < 1 or s > L, L < 1 or L > 32, F < L, rows not a multiple of F * hw,
 *   x NULL, out == x (so a plain op 4 or 5, which carries s = 0, is refused), any bit above the
 *   low byte on ops 0-3; op 5 with y NULL, misaligned or y_f32 != 1; op 4 with y or y_f32 set.
 *   Op 6, VD_ROWS_SPECTRAL, is FreeInit's frequency mix (diffusers' FreeInitMixin
 *   _apply_freq_filter: ifftn(ifftshift(fftshift(fftn(x)) * lpf + fftshift(fftn(noise)) * (1 - lpf))).real
 *   over (frames, height, width)), riding here for the same reason as ops 2-5.  By linearity it is
 *     out = noise + Re(IDFT3(M * DFT3(x - noise))),
 *   M the mask in un-shifted (DFT index) order; taking the real part equals using the
 *   Hermitian-even part of M, so with a Hermitian-even table only the half spectrum kw <= W / 2
 *   is held.  Unlike ops 0-5 ALL DATA ARE FP32 and C % 8 is not required.  The transform is split
 *   into five axis passes, op = VD_ROWS_SPECTRAL | VD_ROWS_SPEC_PASS(p), p = 1..5 (the low byte is
 *   the op), so that the complex scratch is the caller's and travels through the pointer slots:
 *   the library still allocates nothing, never synchronises, and every pass is graph-capturable.
 *   Geometry, the same in every pass: F = y_period frames, H = y_div, W = C, rows = n_vol * F * H
 *   rows of W points, Wh = W / 2 + 1.  S is the scratch: rows rows of 2 * Wh floats, (re, im)
 *   pairs, row stride >= 2 * Wh and even.
 *     p = 1  S[r][kw] = sum_w (x[r][w] - y[r][w]) e^(-2 pi i w kw / W): x the rows to filter, y the
 *            noise rows (y_f32 = 1, ldy its stride), out = S.
 *     p = 2  forward DFT along H, in place: x = out = S (ldx == ldo), y NULL, y_f32 = 0.
 *     p = 3  forward DFT along F, times the table, inverse DFT along F, in one launch, in place:
 *            x = out = S; y the table [F][H][Wh] fp32, contiguous (y_f32 = 1, ldy = Wh), in
 *            un-shifted order and Hermitian-even, M(k) == M(-k mod N) -- the caller's duty, the
 *            entry point cannot check device values.
 *     p = 4  inverse DFT along H, in place, as p = 2.
 *     p = 5  out[r][w] = y[r][w] + (sum_kw m_kw Re(S[r][kw] e^(2 pi i kw w / W))) / (F H W), m = 2
 *            for the bins whose mirror is not stored, else 1: x = S, y the noise rows, out the result
 *            rows.  One correctly rounded division, one addition: a zero spectrum returns y.
 *   Direct O(N^2) DFTs out of LDS.  Twiddles are cos / sin(2 pi ((j k) mod N) / N), the product
 *   reduced mod N in integers, the value rounded once to fp32 from double precision.  A point is
 *   four interleaved fp32 partial sums (n mod 4, ascending n, fmaf per term) combined as
 *   (s0 + s1) + (s2 + s3); no atomics.  A volume's result depends on (F, H, W) and its own data
 *   alone, never on n_vol, the volume's index, the row strides or what the scratch held before.
 *   Sizes: 1 <= F, H, W <= VD_SPECTRAL_MAX (256) each, odd and non-power-of-two included.
 *   VD_EINVAL, before any launch: p outside 1..5 (a plain op 6 carries p = 0; any bit above the
 *   pass byte makes p > 5); a size outside the limit; rows not a multiple of F * H; x or out NULL
 *   or not 16-byte aligned; out == x on p = 1, 5; out != x or ldo != ldx on p = 2..4; y NULL, not
 *   16-byte aligned or y_f32 != 1 on p = 1, 3, 5; y or y_f32 set on p = 2, 4; ldy != Wh on p = 3;
 *   a row stride shorter than its row (W for x / y / out rows, 2 * Wh for S) or an odd S stride.
 *   Op 7, VD_ROWS_CTRL_ADD, is ControlNet's residual injection (diffusers' UNet forward adds the
 *   scaled zero-conv outputs to the down-block skips and to the mid block's output), riding here
 *   for the same reason as ops 2-6.  op = VD_ROWS_CTRL_ADD | VD_ROWS_CTRL_COL(i), i the table
 *   column (the low byte is the op):
 *     out[r][c] = bf16( fmaf(s, float(x[r][c]), float(out[r][c])) ),  r < rows, c < C,
 *     s = tab[clamp(step, 0, y_period - 1) * ldy + i].
 *   x = the control residual, bf16 rows of stride ldx; out = the skip, bf16 rows of stride ldo,
 *   read and written in place (it may be a column or row slice of a wider buffer).  y = one fp32
 *   control block in DEVICE memory, 16-byte aligned, y_f32 == 1: floats 0..3 are a header whose
 *   word 0 is the int32 step index (the denoising loop's device step counter lives there, as the
 *   LCM noise lives in coef: the kernel needs no extra pointer; words 1..3 are ignored), then
 *   tab, y_period rows of ldy floats.  y_div is not read.  Step, scale and data are all read
 *   inside the launch only, so a captured step replays over the whole schedule with the scale
 *   changing between replays (control_guidance_start / end) and per residual (guess mode).
 *   One fused multiply-add in fp32 and one rounding to bf16 per element, 16-byte chunks, no
 *   atomics; s == 0 returns out as it was (a -0 may come back as +0).
 *   VD_EINVAL, before any launch: x, y or out NULL or not 16-byte aligned; y_f32 != 1; ldy
 *   outside 1..64; i >= ldy; any bit above the column byte; y_period < 1; C % 8; x == out; y not
 *   inside a device allocation (hipPointerGetAttributes: every thread reads the step word through
 *   it, and a plain op 7 with host operands stays refused as it was before the op existed).
 *   Op 8, VD_ROWS_SPARSE_COND, builds SparseCtrl's condition rows (diffusers'
 *   AnimateDiffSparseControlNetPipeline.prepare_sparse_control_conditioning: zeros, the key frames
 *   assigned at controlnet_frame_indices, and a mask channel that is 1 on those frames), riding
 *   here for the same reason as ops 2-7.  op = VD_ROWS_SPARSE_COND | VD_ROWS_SPARSE_CH(cc), cc the
 *   number of condition channels, 1..7 (the low byte is the op; 4 = a VAE latent, 3 = pixels).
 *   The output is the packed NHWC rows the conv loaders take: C == 8 bf16 columns.  Geometry:
 *   F = y_period frames, hw = y_div positions per frame, K = ldy key frames per video, rows =
 *   B * F * hw OUTPUT rows.  x = bf16 rows of stride ldx >= 8, key frame k of video b at rows
 *   (b * K + k) * hw + p; only columns < cc are read, whatever columns cc..7 hold never reaches
 *   the output.  y = K int32 frame indices in DEVICE memory, 4-byte aligned, y_f32 == 1 (4-byte
 *   words, as op 7's step word), read inside the launch only.  For video b, frame f, position p,
 *   with k* the LARGEST k whose idx[k] == f (the last assignment wins, as in torch indexing):
 *     out[(b * F + f) * hw + p] = { x[(b * K + k*) * hw + p][0..cc), bf16 1.0, +0 ... }  if k* exists,
 *                                 { +0 x 8 }                                           otherwise.
 *   The cc channels are copied bit for bit.  An index outside [0, F) matches no frame (the host
 *   wrapper refuses it).  A gather: every output row looks its frame up in a table of the K
 *   indices; no scatter, no atomics, one 16-byte store per row, every output element written.
 *   VD_EINVAL, before any launch: cc == 0 (a plain op 8) or cc > 7 or any bit above the channel
 *   byte; C != 8; K or F outside 1..256; hw < 1; rows not a multiple of F * hw; x or out NULL or
 *   not 16-byte aligned; out == x; ldx or ldo below 8 or not a multiple of 8; y NULL, misaligned,
 *   y_f32 != 1 or not inside a device allocation (hipPointerGetAttributes, as op 7).
 *   Op 9, VD_ROWS_PROMPT_LERP, is FreeNoise's prompt travel (diffusers'
 *   AnimateDiffFreeNoiseMixin._encode_prompt_free_noise with its default linear
 *   prompt_interpolation_callback: the key prompts' embeddings interpolated frame by frame), riding
 *   here for the same reason as ops 2-8.  The op word is the plain op: nothing rides above the low
 *   byte.  Geometry, as op 8's: F = y_period frames, L = y_div tokens per prompt, K = ldy key prompts
 *   per video, rows = B * F * L OUTPUT rows of C columns.  x = bf16 key rows of stride ldx >= C, key
 *   k of video b, token l at row (b * K + k) * L + l.  y = K int32 frame indices in DEVICE memory,
 *   4-byte aligned, y_f32 == 1, read inside the launch only, shared by all videos; they must be
 *   strictly increasing with idx[0] == 0 and idx[K - 1] == F - 1 (the host wrapper's duty: the
 *   entry point cannot check device values).  For video b, frame f, token l, with k the LARGEST
 *   index whose idx[k] <= f:
 *     out[(b * F + f) * L + l] = x[(b * K + k) * L + l], bit for bit,            if f == idx[k],
 *                                bf16( fmaf(w, B, (1.0f - w) * A) ) per element  otherwise,
 *     A = float(x[(b * K + k) * L + l]), B = float(x[(b * K + k + 1) * L + l]),
 *     w = float(f - idx[k]) / float(idx[k + 1] - idx[k]), one correctly rounded fp32 division;
 *   1.0f - w and (1.0f - w) * A are rounded to fp32, then one fused multiply-add and one rounding
 *   to bf16.  16-byte chunks, no atomics, every output element written; out may be a column slice
 *   of a wider buffer.  The result of video b depends on its own keys and the table alone.  A
 *   table that breaks the contract never makes the kernel read outside x: k and k + 1 are clamped
 *   into [0, K - 1] before addressing (the values are then unspecified).
 *   VD_EINVAL, before any launch: any bit above the op byte; K or F outside 1..256; L < 1; rows not
 *   a multiple of F * L; C % 8; x or out NULL or not 16-byte aligned; out == x; ldx or ldo below C
 *   or not a multiple of 8; y NULL, misaligned, y_f32 != 1 or not inside a device allocation
 *   (hipPointerGetAttributes, as ops 7 and 8).
 * vd_upsample_nearest2x: rows of n_img h x w images -> rows of their nearest x2 upsample
 *   (Upsample2D's F.interpolate(scale_factor=2.0, mode="nearest")). */
enum {
  VD_ROWS_ADD = 0,
  VD_ROWS_SILU = 1,
  VD_ROWS_FREEU_FILTER = 2,
  VD_ROWS_SCALE = 3,
  VD_ROWS_WIN_GATHER = 4,
  VD_ROWS_WIN_MERGE = 5,
  VD_ROWS_SPECTRAL = 6,
  VD_ROWS_CTRL_ADD = 7,
  VD_ROWS_SPARSE_COND = 8,
  VD_ROWS_PROMPT_LERP = 9
};
#define VD_ROWS_WIN_STRIDE(s) ((s) << 8)
#define VD_ROWS_SPEC_PASS(p) ((p) << 8)
#define VD_ROWS_CTRL_COL(i) ((i) << 8)
#define VD_ROWS_SPARSE_CH(cc) ((cc) << 8)
#define VD_SPECTRAL_MAX 256
int vd_rows_eltwise(int32_t op, const void* x, int64_t ldx, const void* y, int64_t ldy, int32_t y_f32,
                    int64_t y_div, int64_t y_period, int64_t rows, int64_t C, void* out, int64_t ldo,
                    vd_stream_t stream);
int vd_upsample_nearest2x(const void* x, int64_t ldx, int64_t n_img, int64_t h, int64_t w, int64_t C,
                          void* out, int64_t ldo, vd_stream_t stream);

/* ---- DiT-style denoiser (BASELINE config 5; build-defined model,
 * no reference counterpart — oracle/dit_ref.py is its restatement) ----
 * vd_patchify: latents fp32 (B,C,F,H,W) / in_div -> token rows bf16 [(b,f,hp,wp)][kpad],
 *   k = (c*p + ph)*p + pw (Conv3d (1,p,p) patch-embed flattening), zero-padded; dup = 2
 *   writes the CFG copy after the first B*F*(H/p)*(W/p) rows.
 * vd_unpatchify: token rows fp32 [(n,hp,wp)][(ph,pw,c)] -> NHWC pixel rows fp32 [(n,h,w)][c].
 * vd_rope_qk: rotary embedding (rotate-half pairs) in place on columns [0, ncols) of token
 *   rows, head width d; mode 0 = spatial 2-D (first d/2 dims by row h, last d/2 by column
 *   w), mode 1 = temporal 1-D (frame f); token r = ((b*F + f)*Hp + h)*Wp + w.
 * vd_res_ln_mod: per row (b = row / rows_per_b): xn = x + gate[b]*y (y, gate optional),
 *   x_out = xn (optional, may alias x), h = LN(xn, eps; no affine)*(1 + scale[b]) + shift[b]
 *   (shift/scale optional); C <= 2048, C % 8 == 0; gate/shift/scale fp32 rows of ld_mod. */
int vd_patchify(const float* lat, int64_t B, int64_t C, int64_t F, int64_t H, int64_t W,
                int32_t p, int32_t dup, float in_div, void* out, int64_t kpad, vd_stream_t stream);
int vd_unpatchify(const float* src, int64_t ld_src, int64_t n_img, int64_t H, int64_t W,
                  int32_t p, int32_t C, float* dst, vd_stream_t stream);
int vd_rope_qk(void* x, int64_t ld, int64_t rows, int32_t ncols, int32_t d, int32_t mode,
               int64_t F, int64_t Hp, int64_t Wp, float theta, vd_stream_t stream);
int vd_res_ln_mod(const void* x, int64_t ldx, const void* y, int64_t ldy, const float* gate,
                  const float* shift, const float* scale, int64_t ld_mod, int64_t rows_per_b,
                  void* x_out, int64_t ldxo, void* h, int64_t ldh, int64_t rows, int64_t C,
                  float eps, vd_stream_t stream);

/* fp8 spatial self-attention, d = 64 (BASELINE config 5 "fp8 MFMA QK^T/PV"; the DiT's
 * spatial blocks): block-scaled v_mfma_scale_f32_32x32x64_f8f6f4, OCP e4m3 operands.
 * vd_attention_fp8_quant: q/k/v bf16 rows (column slices of the fused QKV buffer) ->
 *   q8/k8 fp8 rows [batch*s][ld8] (ld8 >= heads*64, % 16) with one E8M0 scale byte per
 *   (row, head) in qs/ks [batch*s][heads]; vt8 = V^T fp8 [batch*heads][64][skv] with the keys
 *   of every 64-key tile in the MFMA's k-slot order, vs = one E8M0 per (image, head, tile).
 *   q_scale multiplies q before it is quantized (round 5): pass scale * log2(e) and call
 *   vd_attention_fp8 with scale = 1 / log2(e) to fold the softmax scale into q8 (the kernel then
 *   applies no per-score multiply and takes its exp2 argument straight from the MFMA); 1.0 keeps q.
 * vd_attention_fp8: softmax(scale * Q K^T) V from those operands (Q the dequantized q8) ->
 *   bf16 rows o (column h*64 of head h).  sq % 32 == 0, skv % 64 == 0.
 * vd_attention_fp8_quant_rope: vd_attention_fp8_quant for the DiT's spatial blocks with
 *   vd_rope_qk mode 0 (s = Hp*Wp tokens per image) applied to q and k in fp32 inside the
 *   quantization pass (q/k are read un-rotated and left unchanged). */
int vd_attention_fp8_quant(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                           int64_t ldv, int64_t batch, int32_t heads, int64_t sq, int64_t skv,
                           int32_t d, void* q8, void* k8, int64_t ld8, void* vt8, void* qs, void* ks,
                           void* vs, float q_scale, vd_stream_t stream);
int vd_attention_fp8_quant_rope(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                int64_t ldv, int64_t batch, int32_t heads, int64_t s, int32_t d,
                                int64_t Hp, int64_t Wp, float theta, void* q8, void* k8, int64_t ld8,
                                void* vt8, void* qs, void* ks, void* vs, float q_scale,
                                vd_stream_t stream);
int vd_attention_fp8(const void* q8, const void* k8, int64_t ld8, const void* qs, const void* ks,
                     const void* vt8, const void* vs, void* o, int64_t ldo, int64_t batch,
                     int32_t heads, int64_t sq, int64_t skv, int32_t d, float scale,
                     vd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VDIFF_H */
