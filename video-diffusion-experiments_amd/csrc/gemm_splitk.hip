// The reduce launch behind a split-K v2 / v3 / v5 GEMM: every K slice wrote its fp32 slab to the
// workspace (slab s at ws + s * M * N floats); v6 reduces its slabs inside its own kernel.
#include "gemm_common.h"

namespace {

// Sum the split-K slabs and apply the GEMM epilogue (4 output columns per thread).
// Index math in 32 bits (M * N < 2^31, checked by vd_gemm: M * ldc): a 64-bit division per element
// was most of this memory-bound kernel's instructions (round 3).
__global__ __launch_bounds__(256) void gemm_splitk_reduce(const vd_gemm_desc d, int split) {
  const int64_t M = d.M, N = d.N;
  const bool geglu = d.act == VD_ACT_GEGLU;
  const int64_t nout = geglu ? N / 2 : N;
  const int total = (int)(M * (nout / 4));
  const Div dq((int)(nout / 4)), drb(d.rowbias ? (int)d.rb_div : 1);
  const float* ws = (const float*)d.ws;
  const Rev3 perm(d.M, d.rmap_n1, d.rmap_n2, d.rmap_inner);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int m32 = dq(i);
    const int64_t m = m32, mo = perm(m32);  // slab row, output / residual row
    const int64_t o = (int64_t)(i - m32 * (int)(nout / 4)) * 4;
    float o4[4];
    if (geglu) {
      const int64_t nh = (o / 16) * 32 + (o % 16), ng = nh + 16;
      float h[4] = {0, 0, 0, 0}, g[4] = {0, 0, 0, 0};
      for (int sp = 0; sp < split; ++sp) {
        const float4 a = *(const float4*)(ws + (sp * M + m) * N + nh);
        const float4 b = *(const float4*)(ws + (sp * M + m) * N + ng);
        h[0] += a.x; h[1] += a.y; h[2] += a.z; h[3] += a.w;
        g[0] += b.x; g[1] += b.y; g[2] += b.z; g[3] += b.w;
      }
      if (d.bias) {
        const float4 a = *(const float4*)(d.bias + nh);
        const float4 b = *(const float4*)(d.bias + ng);
        h[0] += a.x; h[1] += a.y; h[2] += a.z; h[3] += a.w;
        g[0] += b.x; g[1] += b.y; g[2] += b.z; g[3] += b.w;
      }
      for (int j = 0; j < 4; ++j) o4[j] = h[j] * gelu_erf(g[j]);
    } else {
      float v[4] = {0, 0, 0, 0};
      for (int sp = 0; sp < split; ++sp) {
        const float4 a = *(const float4*)(ws + (sp * M + m) * N + o);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
      }
      if (d.bias) {
        const float4 a = *(const float4*)(d.bias + o);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
      }
      if (d.rowbias) {
        const float4 a = *(const float4*)(d.rowbias + (int64_t)drb(m32) * d.ld_rb + o);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
      }
      if (act_is_pw(d.act))
        for (int j = 0; j < 4; ++j) v[j] = act_pw(d.act, v[j]);
      if (d.res) {
        const uint2 r = *(const uint2*)((const bf16_t*)d.res + mo * d.ld_res + o);
        v[0] += bf_lo(r.x); v[1] += bf_hi(r.x); v[2] += bf_lo(r.y); v[3] += bf_hi(r.y);
      }
      for (int j = 0; j < 4; ++j) o4[j] = v[j];
    }
    if (d.out_f32)
      *(float4*)((float*)d.out + mo * d.ldc + o) = make_float4(o4[0], o4[1], o4[2], o4[3]);
    else
      *(uint2*)((bf16_t*)d.out + mo * d.ldc + o) = make_uint2(pack2(o4[0], o4[1]), pack2(o4[2], o4[3]));
  }
}

}  // namespace

namespace vdgemm {

int launch_splitk_reduce(const vd_gemm_desc& d, int split, hipStream_t s) {
  const int64_t work = d.M * ((d.act == VD_ACT_GEGLU ? d.N / 2 : d.N) / 4);
  const int64_t blocks = (work + 255) / 256;
  hipLaunchKernelGGL(gemm_splitk_reduce, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, d, split);
  return vd_launch_status();
}

}  // namespace vdgemm
