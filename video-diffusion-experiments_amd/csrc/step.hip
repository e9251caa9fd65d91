// Step glue: timestep embedding, latent layout conversion, the fused
// CFG-combine + DDIM update, and the row-block transpose used by the frame
// <-> position re-shard.  All HBM-bound elementwise kernels.
//
// vd_ddim_cfg_step fuses SURVEY.md §8a a1 (eps = e_u + g (e_c - e_u)) and a13
// (diffusers:DDIMScheduler.step, eta 0, epsilon prediction — App. A.7):
//   x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t);  x <- sqrt(a_p) x0 + sqrt(1-a_p) eps
// reading the conv_out rows directly (NHWC fp32) and, optionally, writing the
// next step's packed bf16 UNet input (the CFG cat([x, x])) in the same pass.
// Coefficients come from a device table indexed by a device step counter so a
// captured hipGraph of one step can be replayed for every timestep.  With VD_STEP_LCM in ncfg
// the same entry point launches the LCMScheduler update, whose per-step noise follows the
// coefficient rows in the same device buffer (lcm_cfg_kernel); with VD_STEP_DPM the
// DPMSolverMultistepScheduler update, whose history travels in x0_out (dpm_cfg_kernel); with
// VD_STEP_UNIPC the UniPCMultistepScheduler update, corrector and predictor in one pass, whose
// three state slabs travel in x0_out (unipc_cfg_kernel).  vd_euler_cfg_step likewise takes
// VD_STEP_ANCESTRAL: the EulerAncestralDiscreteScheduler update, its per-step noise behind the
// rows as LCM's (euler_a_cfg_kernel).
#include "common.h"

namespace {

constexpr int NT = 256;

// fp32 quotient, correctly rounded (via double: 53 >= 2*24 + 2, so the second rounding is
// innocuous) — the GPU's default f32 division is a reciprocal-refinement sequence
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }


// Step index into a device table of n entries, clamped to [0, n-1]: a graph replayed past the
// end of its schedule (run(n) beyond n_steps without reset()) keeps reading the last row
// instead of memory past the table (the host loops raise before that happens).
__device__ __forceinline__ int table_row(const int32_t* step_idx, int64_t n) {
  int st = step_idx ? *step_idx : 0;
  st = st < 0 ? 0 : st;
  return (int64_t)st < n ? st : (int)(n - 1);
}

__global__ void timestep_embed_kernel(const float* ts, int64_t n_ts, const int32_t* step_idx, int64_t B, int dim,
                                      bf16_t* out) {
  const int half = dim / 2;
  const int64_t total = B * dim;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t b = i / dim;
    const int c = (int)(i - b * dim);
    const float t = step_idx ? ts[table_row(step_idx, n_ts)] : ts[b];
    const int j = c < half ? c : c - half;
    // diffusers get_timestep_embedding: exp(-ln(1e4) * j / half); flip -> [cos, sin]
    const float freq = expf(-9.210340371976184f * (float)j / (float)half);
    const float arg = t * freq;
    out[i] = f2bf(c < half ? cosf(arg) : sinf(arg));
  }
}

__global__ void pack_latents_kernel(const float* x, int64_t B, int64_t C, int64_t F, int64_t HW,
                                    int dup, bf16_t* out, int64_t cpad, float in_div) {
  // out row r = ((d*B + b)*F + f)*HW + p, channel c  <-  x[b][c][f][p] / in_div
  const int64_t rows = dup * B * F * HW;
  const int64_t total = rows * cpad;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t r = i / cpad;
    const int64_t c = i - r * cpad;
    const int64_t p = r % HW;
    const int64_t f = (r / HW) % F;
    const int64_t b = (r / (HW * F)) % B;
    float val = 0.f;
    if (c < C) val = in_div == 1.f ? x[((b * C + c) * F + f) * HW + p] : div_rn(x[((b * C + c) * F + f) * HW + p], in_div);
    out[i] = f2bf(val);
  }
}

__global__ void unpack_kernel(const void* src, int src_f32, int64_t ld, int64_t B, int64_t C,
                              int64_t F, int64_t HW, float* dst) {
  const int64_t total = B * C * F * HW;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t p = i % HW;
    const int64_t f = (i / HW) % F;
    const int64_t c = (i / (HW * F)) % C;
    const int64_t b = i / (HW * F * C);
    const int64_t r = (b * F + f) * HW + p;
    dst[i] = src_f32 ? ((const float*)src)[r * ld + c] : bf2f(((const bf16_t*)src)[r * ld + c]);
  }
}

// next_in is the whole packed UNet input, as vd_pack_latents writes it: `copies` copies of the
// batch (one per guidance branch), the channel padding [C, cpad) of every row zero.  The thread
// of the row's channel 0 writes the padding, so a next_in that was never packed before (a fresh
// allocation) is fully defined after the step.
__device__ __forceinline__ void write_next_in(bf16_t* next_in, bf16_t v, int64_t r, int64_t c,
                                              int64_t half_rows, int copies, int64_t C, int64_t cpad) {
  for (int k = 0; k < copies; ++k) {
    bf16_t* row = next_in + (r + k * half_rows) * cpad;
    row[c] = v;
    if (c == 0)
      for (int64_t cc = C; cc < cpad; ++cc) row[cc] = 0;
  }
}

// The guided eps of one element, shared by the four step kernels.  eps holds ncfg branches of
// half_rows rows each.  Without PAG (pag == nullptr): ncfg 1 is the row itself, ncfg 2 is
// [uncond; cond] and e = e_u + g (e_c - e_u).  With PAG (s = pag[st], read by the caller):
// ncfg 3 is [uncond; cond; perturbed], e = (e_u + g (e_c - e_u)) + s (e_c - e_p); ncfg 2 is
// [cond; perturbed], e = e_c + s (e_c - e_p).  fp32, one rounding per operation.
__device__ __forceinline__ float guided_eps(const float* eps, int64_t ld_eps, int64_t r, int64_t c,
                                            int64_t half_rows, int ncfg, float g, bool pag, float s) {
#pragma clang fp contract(off)
  const float e0 = eps[r * ld_eps + c];
  if (ncfg == 1) return e0;
  const float e1 = eps[(r + half_rows) * ld_eps + c];
  if (!pag) return e0 + g * (e1 - e0);
  if (ncfg == 2) return e0 + s * (e0 - e1);
  const float ep = eps[(r + 2 * half_rows) * ld_eps + c];
  const float e = e0 + g * (e1 - e0);
  return e + s * (e1 - ep);
}

// fp32 in diffusers' operation order with one rounding per operation (no contraction,
// correctly rounded division), as torch's separate fp32 ops: bit-exact vs oracle/ddim_ref.py.
__global__ void ddim_cfg_kernel(const float* eps, int64_t ld_eps, int ncfg, float g, float* lat,
                                int64_t B, int64_t C, int64_t F, int64_t HW, const float* coef,
                                int64_t n_coef, const int32_t* step_idx, float* x0_out, bf16_t* next_in,
                                int64_t cpad, const float* pag) {
#pragma clang fp contract(off)
  const int st = table_row(step_idx, n_coef);
  const float pag_s = pag ? pag[st] : 0.f;
  const float sat = coef[4 * st + 0], s1at = coef[4 * st + 1];
  const float sap = coef[4 * st + 2], s1ap = coef[4 * st + 3];
  const int64_t total = B * C * F * HW;
  const int64_t half_rows = B * F * HW;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t p = i % HW;
    const int64_t f = (i / HW) % F;
    const int64_t c = (i / (HW * F)) % C;
    const int64_t b = i / (HW * F * C);
    const int64_t r = (b * F + f) * HW + p;
    const float e = guided_eps(eps, ld_eps, r, c, half_rows, ncfg, g, pag != nullptr, pag_s);
    const float x = lat[i];
    const float x0 = div_rn(x - s1at * e, sat);
    const float xn = sap * x0 + s1ap * e;
    lat[i] = xn;
    if (x0_out) x0_out[i] = x0;
    if (next_in) write_next_in(next_in, f2bf(xn), r, c, half_rows, ncfg, C, cpad);
  }
}

// CFG combine + diffusers:EulerDiscreteScheduler.step (s_churn = 0, epsilon
// prediction), in diffusers' fp32 operation order:
//   x0 = x - sigma*eps;  d = (x - x0) / sigma;  x <- x + d * (sigma_next - sigma)
// and the next step's UNet input = scale_model_input(x, sigma_next) = x / sqrt(sigma_next^2 + 1)
// (coef[4*st] = {sigma, sigma_next, sqrt(sigma_next^2 + 1), 0}).
__global__ void euler_cfg_kernel(const float* eps, int64_t ld_eps, int ncfg, float g, float* lat,
                                 int64_t B, int64_t C, int64_t F, int64_t HW, const float* coef,
                                 int64_t n_coef, const int32_t* step_idx, float* x0_out, bf16_t* next_in,
                                 int64_t cpad, const float* pag) {
#pragma clang fp contract(off)  // one rounding per operation, as torch's separate fp32 ops
  const int st = table_row(step_idx, n_coef);
  const float pag_s = pag ? pag[st] : 0.f;
  const float sig = coef[4 * st + 0], sig_n = coef[4 * st + 1], in_div = coef[4 * st + 2];
  const float dt = sig_n - sig;
  const int64_t total = B * C * F * HW;
  const int64_t half_rows = B * F * HW;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t p = i % HW;
    const int64_t f = (i / HW) % F;
    const int64_t c = (i / (HW * F)) % C;
    const int64_t b = i / (HW * F * C);
    const int64_t r = (b * F + f) * HW + p;
    const float e = guided_eps(eps, ld_eps, r, c, half_rows, ncfg, g, pag != nullptr, pag_s);
    const float x = lat[i];
    const float x0 = x - sig * e;
    const float d = div_rn(x - x0, sig);
    const float xn = x + d * dt;
    lat[i] = xn;
    if (x0_out) x0_out[i] = x0;
    if (next_in) write_next_in(next_in, f2bf(div_rn(xn, in_div)), r, c, half_rows, ncfg, C, cpad);
  }
}

// CFG combine + diffusers:EulerAncestralDiscreteScheduler.step (epsilon prediction), in diffusers'
// fp32 operation order (vd_euler_cfg_step with VD_STEP_ANCESTRAL in ncfg):
//   x0 = x - sigma*eps;  d = (x - x0) / sigma;  x <- x + d * (sigma_down - sigma)
//   x <- x + noise * sigma_up                    (only where sigma_up != 0)
// and the next step's UNet input = x / sqrt(sigma_to^2 + 1).  coef holds n_coef rows of 4 floats
// {sigma, sigma_down, sqrt(sigma_to^2 + 1), sigma_up} — Euler's row with sigma_next replaced and
// its unused zero filled — and, from float 4 * n_coef on, n_coef noise slabs of B*C*F*HW floats in
// latent order, as LCM's.  Row and noise are read here by the device step index, so one captured
// launch serves the whole schedule.  A slab whose row has sigma_up == 0 (the last step of every
// schedule) is never read, so an Euler table under the flag gives euler_cfg_kernel's result.
__global__ void euler_a_cfg_kernel(const float* eps, int64_t ld_eps, int ncfg, float g, float* lat,
                                   int64_t B, int64_t C, int64_t F, int64_t HW, const float* coef,
                                   int64_t n_coef, const int32_t* step_idx, float* x0_out, bf16_t* next_in,
                                   int64_t cpad, const float* pag) {
#pragma clang fp contract(off)  // one rounding per operation, as torch's separate fp32 ops
  const int st = table_row(step_idx, n_coef);
  const float pag_s = pag ? pag[st] : 0.f;
  const float sig = coef[4 * st + 0], sig_d = coef[4 * st + 1], in_div = coef[4 * st + 2];
  const float sig_up = coef[4 * st + 3];
  const bool add_noise = sig_up != 0.f;
  const float dt = sig_d - sig;
  const int64_t total = B * C * F * HW;
  const int64_t half_rows = B * F * HW;
  const float* noise = coef + 4 * n_coef + (int64_t)st * total;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t p = i % HW;
    const int64_t f = (i / HW) % F;
    const int64_t c = (i / (HW * F)) % C;
    const int64_t b = i / (HW * F * C);
    const int64_t r = (b * F + f) * HW + p;
    const float e = guided_eps(eps, ld_eps, r, c, half_rows, ncfg, g, pag != nullptr, pag_s);
    const float x = lat[i];
    const float x0 = x - sig * e;
    const float d = div_rn(x - x0, sig);
    float xn = x + d * dt;
    if (add_noise) xn = xn + noise[i] * sig_up;
    lat[i] = xn;
    if (x0_out) x0_out[i] = x0;
    if (next_in) write_next_in(next_in, f2bf(div_rn(xn, in_div)), r, c, half_rows, ncfg, C, cpad);
  }
}

// CFG combine + diffusers:LCMScheduler.step (epsilon prediction), in diffusers' fp32 operation
// order (vd_ddim_cfg_step with VD_STEP_LCM in ncfg):
//   x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t);  den = c_out x0 + c_skip x
//   x <- add_noise ? sqrt(a_p) den + sqrt(1-a_p) noise : den
// coef holds n_coef rows of 8 floats {sqrt(a_t), sqrt(1-a_t), sqrt(a_p), sqrt(1-a_p), c_skip,
// c_out, add_noise, 0} and, from float 8 * n_coef on, n_coef noise slabs of B*C*F*HW floats in
// latent order.  Row, branch and noise are all read here by the device step index, so one
// captured launch serves the whole schedule.  A slab whose row has add_noise == 0 is never read.
__global__ void lcm_cfg_kernel(const float* eps, int64_t ld_eps, int ncfg, float g, float* lat,
                               int64_t B, int64_t C, int64_t F, int64_t HW, const float* coef,
                               int64_t n_coef, const int32_t* step_idx, float* x0_out, bf16_t* next_in,
                               int64_t cpad, const float* pag) {
#pragma clang fp contract(off)  // one rounding per operation, as torch's separate fp32 ops
  const int st = table_row(step_idx, n_coef);
  const float pag_s = pag ? pag[st] : 0.f;
  const float* row = coef + 8 * (int64_t)st;
  const float sat = row[0], s1at = row[1], sap = row[2], s1ap = row[3];
  const float c_skip = row[4], c_out = row[5];
  const bool add_noise = row[6] != 0.f;
  const int64_t total = B * C * F * HW;
  const int64_t half_rows = B * F * HW;
  const float* noise = coef + 8 * n_coef + (int64_t)st * total;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t p = i % HW;
    const int64_t f = (i / HW) % F;
    const int64_t c = (i / (HW * F)) % C;
    const int64_t b = i / (HW * F * C);
    const int64_t r = (b * F + f) * HW + p;
    const float e = guided_eps(eps, ld_eps, r, c, half_rows, ncfg, g, pag != nullptr, pag_s);
    const float x = lat[i];
    const float x0 = div_rn(x - s1at * e, sat);
    const float den = c_out * x0 + c_skip * x;
    float xn = den;
    if (add_noise) xn = sap * den + s1ap * noise[i];
    lat[i] = xn;
    if (x0_out) x0_out[i] = den;
    if (next_in) write_next_in(next_in, f2bf(xn), r, c, half_rows, ncfg, C, cpad);
  }
}

// CFG combine + diffusers:DPMSolverMultistepScheduler.step (dpmsolver++ and sde-dpmsolver++,
// midpoint, order 1 or 2, epsilon prediction), in diffusers' fp32 operation order
// (vd_ddim_cfg_step with VD_STEP_DPM in ncfg):
//   x0 = (x - sigma_s eps) / alpha_s;  x <- c_x x + c_m0 x0 [+ c_d1 (1/r0) (x0 - m1)] [+ c_noise noise]
// coef holds n_coef rows of 8 floats {alpha_s, sigma_s, c_x, c_m0, c_d1, 1/r0, c_noise, flags}
// (flags: 1.0 second order, 2.0 SDE noise, 3.0 both) and, when any row is an SDE row, n_coef noise
// slabs of B*C*F*HW floats from float 8 * n_coef on.  The deterministic type's two subtracted
// terms are stored negated, so both types share this add-only form (a - c b == a + (-c) b bit for
// bit).  hist (x0_out) is in/out: the previous step's x0 on entry (m1, read only by a second-order
// row), this step's on exit; each thread reads m1[i] before it writes x0[i].
__global__ void dpm_cfg_kernel(const float* eps, int64_t ld_eps, int ncfg, float g, float* lat,
                               int64_t B, int64_t C, int64_t F, int64_t HW, const float* coef,
                               int64_t n_coef, const int32_t* step_idx, float* hist, bf16_t* next_in,
                               int64_t cpad, const float* pag) {
#pragma clang fp contract(off)  // one rounding per operation, as torch's separate fp32 ops
  const int st = table_row(step_idx, n_coef);
  const float pag_s = pag ? pag[st] : 0.f;
  const float* row = coef + 8 * (int64_t)st;
  const float alpha_s = row[0], sigma_s = row[1], c_x = row[2], c_m0 = row[3];
  const float c_d1 = row[4], inv_r0 = row[5], c_noise = row[6];
  const int flags = (int)row[7];
  const bool second = (flags & 1) != 0, sde = (flags & 2) != 0;
  const int64_t total = B * C * F * HW;
  const int64_t half_rows = B * F * HW;
  const float* noise = coef + 8 * n_coef + (int64_t)st * total;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t p = i % HW;
    const int64_t f = (i / HW) % F;
    const int64_t c = (i / (HW * F)) % C;
    const int64_t b = i / (HW * F * C);
    const int64_t r = (b * F + f) * HW + p;
    const float e = guided_eps(eps, ld_eps, r, c, half_rows, ncfg, g, pag != nullptr, pag_s);
    const float x = lat[i];
    const float x0 = div_rn(x - sigma_s * e, alpha_s);
    float xn = c_x * x + c_m0 * x0;
    if (second) {
      const float d1 = inv_r0 * (x0 - hist[i]);
      xn = xn + c_d1 * d1;
    }
    if (sde) xn = xn + c_noise * noise[i];
    lat[i] = xn;
    hist[i] = x0;
    if (next_in) write_next_in(next_in, f2bf(xn), r, c, half_rows, ncfg, C, cpad);
  }
}

// CFG combine + diffusers:UniPCMultistepScheduler.step (predict_x0, bh1 / bh2, solver order 1 or 2,
// epsilon prediction): the corrector of the previous step and the predictor of this one in one
// pass, in diffusers' fp32 operation order (vd_ddim_cfg_step with VD_STEP_UNIPC in ncfg).
// coef holds n_coef rows of 16 floats {alpha_s, sigma_s, c_last, c_m, c_B, rk_c, rho0, rhot, p_x,
// p_m, p_B, rk_p, flags, 0, 0, 0}; flags = 1 the corrector runs + 2 it is second order + 4 the
// predictor is second order.  A slot its row does not use is 0 and is not read: no division by an
// unused rk.  state (x0_out) is in/out, three slabs of B*C*F*HW floats: S0 the latest x0
// prediction, S1 the one before it, S2 `last`, the sample the previous predictor started from.
//   m_t = (x - sigma_s e) / alpha_s
//   corrector:  x_ = c_last S2 - c_m S0;  r = [rho0 (S1 - S0) / rk_c +] rhot (m_t - S0);  xc = x_ - c_B r
//   predictor:  y = p_x xc - p_m m_t [- p_B (0.5 (S0 - m_t) / rk_p)]
//   lat <- y;  S1 <- S0;  S0 <- m_t;  S2 <- xc
// Each thread reads its element of every slab before it writes any.  A flags-0 row (step 0 of a
// run) reads no slab — it starts the history, S1 <- m_t as well — and only a second-order
// corrector reads S1, so the state needs no clearing between schedules.
__global__ void unipc_cfg_kernel(const float* eps, int64_t ld_eps, int ncfg, float g, float* lat,
                                 int64_t B, int64_t C, int64_t F, int64_t HW, const float* coef,
                                 int64_t n_coef, const int32_t* step_idx, float* state, bf16_t* next_in,
                                 int64_t cpad, const float* pag) {
#pragma clang fp contract(off)  // one rounding per operation, as torch's separate fp32 ops
  const int st = table_row(step_idx, n_coef);
  const float pag_s = pag ? pag[st] : 0.f;
  const float* row = coef + 16 * (int64_t)st;
  const float alpha_s = row[0], sigma_s = row[1], c_last = row[2], c_m = row[3], c_B = row[4];
  const float rk_c = row[5], rho0 = row[6], rhot = row[7];
  const float p_x = row[8], p_m = row[9], p_B = row[10], rk_p = row[11];
  const int flags = (int)row[12];
  const bool corr = (flags & 1) != 0, corr2 = (flags & 2) != 0, pred2 = (flags & 4) != 0;
  const int64_t total = B * C * F * HW;
  const int64_t half_rows = B * F * HW;
  float* S0 = state;
  float* S1 = state + total;
  float* S2 = state + 2 * total;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t p = i % HW;
    const int64_t f = (i / HW) % F;
    const int64_t c = (i / (HW * F)) % C;
    const int64_t b = i / (HW * F * C);
    const int64_t r = (b * F + f) * HW + p;
    const float e = guided_eps(eps, ld_eps, r, c, half_rows, ncfg, g, pag != nullptr, pag_s);
    const float x = lat[i];
    const float m_t = div_rn(x - sigma_s * e, alpha_s);
    const float m0 = flags ? S0[i] : m_t;
    float xc = x;
    if (corr) {
      const float x_ = c_last * S2[i] - c_m * m0;
      const float d_t = m_t - m0;
      float res = rhot * d_t;
      if (corr2) res = rho0 * div_rn(S1[i] - m0, rk_c) + res;
      xc = x_ - c_B * res;
    }
    float y = p_x * xc - p_m * m_t;
    if (pred2) y = y - p_B * (0.5f * div_rn(m0 - m_t, rk_p));
    lat[i] = y;
    S1[i] = m0;
    S0[i] = m_t;
    S2[i] = xc;
    if (next_in) write_next_in(next_in, f2bf(y), r, c, half_rows, ncfg, C, cpad);
  }
}

__global__ void step_advance_kernel(int32_t* step_idx) { *step_idx += 1; }

__global__ void block_transpose_kernel(const bf16_t* src, bf16_t* dst, int64_t nb, int64_t na,
                                       int64_t nc, int64_t width) {
  // dst[((a*nb + b)*nc + c)][:] = src[((b*na + a)*nc + c)][:], 16-byte chunks
  const int64_t wch = width / 8;
  const int64_t total = nb * na * nc * wch;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t ch = i % wch;
    const int64_t drow = i / wch;
    const int64_t c = drow % nc;
    const int64_t ab = drow / nc;
    const int64_t b = ab % nb, a = ab / nb;
    const int64_t srow = (b * na + a) * nc + c;
    *(uint4*)(dst + drow * width + ch * 8) = *(const uint4*)(src + srow * width + ch * 8);
  }
}

unsigned grid_for(int64_t total) {
  const int64_t b = (total + NT - 1) / NT;
  return (unsigned)(b < 16384 ? (b > 0 ? b : 1) : 16384);
}

}  // namespace

extern "C" int vd_timestep_embed(const float* ts, int64_t n_ts, const int32_t* step_idx, int64_t B,
                                 int32_t dim, void* out, vd_stream_t stream) {
  VD_CHECK_ARG(ts && out && B > 0 && dim > 0 && dim % 2 == 0 && n_ts > 0);
  if (!step_idx) VD_CHECK_ARG(n_ts >= B);
  hipLaunchKernelGGL(timestep_embed_kernel, dim3(grid_for(B * dim)), dim3(NT), 0,
                     (hipStream_t)stream, ts, n_ts, step_idx, B, dim, (bf16_t*)out);
  return vd_launch_status();
}

extern "C" int vd_pack_latents(const float* x, int64_t B, int64_t C, int64_t F, int64_t H,
                               int64_t W, int32_t dup, void* out, int64_t cpad, float in_div,
                               vd_stream_t stream) {
  VD_CHECK_ARG(x && out && B > 0 && C > 0 && F > 0 && H > 0 && W > 0 && cpad >= C && dup >= 1 && in_div > 0.f);
  const int64_t total = dup * B * F * H * W * cpad;
  hipLaunchKernelGGL(pack_latents_kernel, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream,
                     x, B, C, F, H * W, dup, (bf16_t*)out, cpad, in_div);
  return vd_launch_status();
}

extern "C" int vd_unpack_nhwc(const void* src, int32_t src_f32, int64_t ld, int64_t B, int64_t C,
                              int64_t F, int64_t H, int64_t W, float* dst, vd_stream_t stream) {
  VD_CHECK_ARG(src && dst && ld >= C && B > 0 && C > 0 && F > 0 && H > 0 && W > 0);
  hipLaunchKernelGGL(unpack_kernel, dim3(grid_for(B * C * F * H * W)), dim3(NT), 0,
                     (hipStream_t)stream, src, src_f32, ld, B, C, F, H * W, dst);
  return vd_launch_status();
}

// VD_STEP_PAG: the low byte is 2 or 3 and coef starts with the n_coef PAG scales, padded to a
// multiple of 4 floats; the scheduler's own layout follows.  Splits coef into the two, or refuses.
static int split_pag_coef(int32_t& ncfg, const float*& coef, int64_t n_coef, const float*& pag) {
  pag = nullptr;
  const bool on = (ncfg & VD_STEP_PAG) != 0;
  ncfg &= ~VD_STEP_PAG;
  if (!on) return VD_OK;
  VD_CHECK_ARG(coef && n_coef > 0 && (ncfg == 2 || ncfg == 3) && ((uintptr_t)coef & 15) == 0);
  pag = coef;
  coef += (n_coef + 3) / 4 * 4;
  return VD_OK;
}

extern "C" int vd_ddim_cfg_step(const float* eps, int64_t ld_eps, int32_t ncfg, float guidance,
                                float* latents, int64_t B, int64_t C, int64_t F, int64_t H,
                                int64_t W, const float* coef, int64_t n_coef, const int32_t* step_idx,
                                float* x0_out, void* next_in, int64_t cpad, vd_stream_t stream) {
  // VD_STEP_LCM / VD_STEP_DPM / VD_STEP_UNIPC ride on ncfg above its low byte; two of them at
  // once, or any other high bit but VD_STEP_PAG, are refused
  const bool lcm = (ncfg & VD_STEP_LCM) != 0, dpm = (ncfg & VD_STEP_DPM) != 0, unipc = (ncfg & VD_STEP_UNIPC) != 0;
  VD_CHECK_ARG(lcm + dpm + unipc <= 1);
  ncfg &= ~(VD_STEP_LCM | VD_STEP_DPM | VD_STEP_UNIPC);
  const float* pag;
  if (const int rc = split_pag_coef(ncfg, coef, n_coef, pag)) return rc;
  VD_CHECK_ARG(eps && latents && coef && n_coef > 0 && ld_eps >= C);
  VD_CHECK_ARG(pag ? (ncfg == 2 || ncfg == 3) : (ncfg == 1 || ncfg == 2));
  if (next_in) VD_CHECK_ARG(cpad >= C);
  if (lcm) {
    VD_CHECK_ARG(B > 0 && C > 0 && F > 0 && H > 0 && W > 0 && ((uintptr_t)coef & 15) == 0);
    hipLaunchKernelGGL(lcm_cfg_kernel, dim3(grid_for(B * C * F * H * W)), dim3(NT), 0,
                       (hipStream_t)stream, eps, ld_eps, ncfg, guidance, latents, B, C, F, H * W,
                       coef, n_coef, step_idx, x0_out, (bf16_t*)next_in, cpad, pag);
    return vd_launch_status();
  }
  if (dpm) {
    // x0_out is the history: required, in/out, and not the latents themselves
    VD_CHECK_ARG(B > 0 && C > 0 && F > 0 && H > 0 && W > 0 && ((uintptr_t)coef & 15) == 0);
    VD_CHECK_ARG(x0_out && x0_out != latents);
    hipLaunchKernelGGL(dpm_cfg_kernel, dim3(grid_for(B * C * F * H * W)), dim3(NT), 0,
                       (hipStream_t)stream, eps, ld_eps, ncfg, guidance, latents, B, C, F, H * W,
                       coef, n_coef, step_idx, x0_out, (bf16_t*)next_in, cpad, pag);
    return vd_launch_status();
  }
  if (unipc) {
    // x0_out is the state: required, in/out, three slabs of the latents' size that do not overlap them
    VD_CHECK_ARG(B > 0 && C > 0 && F > 0 && H > 0 && W > 0 && ((uintptr_t)coef & 15) == 0);
    const int64_t total = B * C * F * H * W;
    VD_CHECK_ARG(x0_out && !((uintptr_t)x0_out < (uintptr_t)(latents + total) &&
                             (uintptr_t)latents < (uintptr_t)(x0_out + 3 * total)));
    hipLaunchKernelGGL(unipc_cfg_kernel, dim3(grid_for(total)), dim3(NT), 0,
                       (hipStream_t)stream, eps, ld_eps, ncfg, guidance, latents, B, C, F, H * W,
                       coef, n_coef, step_idx, x0_out, (bf16_t*)next_in, cpad, pag);
    return vd_launch_status();
  }
  hipLaunchKernelGGL(ddim_cfg_kernel, dim3(grid_for(B * C * F * H * W)), dim3(NT), 0,
                     (hipStream_t)stream, eps, ld_eps, ncfg, guidance, latents, B, C, F, H * W,
                     coef, n_coef, step_idx, x0_out, (bf16_t*)next_in, cpad, pag);
  return vd_launch_status();
}

extern "C" int vd_euler_cfg_step(const float* eps, int64_t ld_eps, int32_t ncfg, float guidance,
                                 float* latents, int64_t B, int64_t C, int64_t F, int64_t H,
                                 int64_t W, const float* coef, int64_t n_coef, const int32_t* step_idx,
                                 float* x0_out, void* next_in, int64_t cpad, vd_stream_t stream) {
  // VD_STEP_PAG and VD_STEP_ANCESTRAL are the flags Euler takes; VD_STEP_LCM / VD_STEP_DPM /
  // VD_STEP_UNIPC and any other high bit fail the low-byte check, with or without them
  const bool ancestral = (ncfg & VD_STEP_ANCESTRAL) != 0;
  ncfg &= ~VD_STEP_ANCESTRAL;
  const float* pag;
  if (const int rc = split_pag_coef(ncfg, coef, n_coef, pag)) return rc;
  VD_CHECK_ARG(eps && latents && coef && n_coef > 0 && ld_eps >= C);
  VD_CHECK_ARG(pag ? (ncfg == 2 || ncfg == 3) : (ncfg == 1 || ncfg == 2));
  if (next_in) VD_CHECK_ARG(cpad >= C);
  if (ancestral) {
    VD_CHECK_ARG(B > 0 && C > 0 && F > 0 && H > 0 && W > 0 && ((uintptr_t)coef & 15) == 0);
    hipLaunchKernelGGL(euler_a_cfg_kernel, dim3(grid_for(B * C * F * H * W)), dim3(NT), 0,
                       (hipStream_t)stream, eps, ld_eps, ncfg, guidance, latents, B, C, F, H * W,
                       coef, n_coef, step_idx, x0_out, (bf16_t*)next_in, cpad, pag);
    return vd_launch_status();
  }
  hipLaunchKernelGGL(euler_cfg_kernel, dim3(grid_for(B * C * F * H * W)), dim3(NT), 0,
                     (hipStream_t)stream, eps, ld_eps, ncfg, guidance, latents, B, C, F, H * W,
                     coef, n_coef, step_idx, x0_out, (bf16_t*)next_in, cpad, pag);
  return vd_launch_status();
}

extern "C" int vd_step_advance(int32_t* step_idx, vd_stream_t stream) {
  VD_CHECK_ARG(step_idx);
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_idx);
  return vd_launch_status();
}

extern "C" int vd_block_transpose(const void* src, void* dst, int64_t nb, int64_t na, int64_t nc,
                                  int64_t width, vd_stream_t stream) {
  VD_CHECK_ARG(src && dst && src != dst && width % 8 == 0 && nb > 0 && na > 0 && nc > 0);
  VD_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0);
  hipLaunchKernelGGL(block_transpose_kernel, dim3(grid_for(nb * na * nc * (width / 8))), dim3(NT), 0,
                     (hipStream_t)stream, (const bf16_t*)src, (bf16_t*)dst, nb, na, nc, width);
  return vd_launch_status();
}

extern "C" const char* vd_strerror(int code) {
  switch (code) {
    case VD_OK: return "ok";
    case VD_EINVAL: return "vdiff: invalid argument (shape/stride/alignment)";
    case VD_EUNSUPPORTED: return "vdiff: unsupported parameter (no compiled variant)";
    case VD_ERCCL: return "vdiff: RCCL call failed";
    default: return hipGetErrorString((hipError_t)code);
  }
}

extern "C" int vd_version(void) { return 6; }  // 6: vd_gn_finalize_g_ranks (round 6); 5: vd_gemm_desc rmap_* / ln_fold_*, vd_gemm_plan, vd_gn_apply_rev3, fp8 q_scale (round 5)

#ifndef VD_BUILD_HASH
#define VD_BUILD_HASH "unhashed"
#endif
// Content hash of the sources + flags this library was built from (build_ext.py);
// vdiff._lib refuses to load a library whose hash differs from the tree's sources.
extern "C" const char* vd_build_hash(void) { return VD_BUILD_HASH; }

#ifndef VD_BUILD_ARCH
#define VD_BUILD_ARCH "gfx950"
#endif
// The --offload-arch the library was compiled for (kept out of the content hash).
extern "C" const char* vd_build_arch(void) { return VD_BUILD_ARCH; }
