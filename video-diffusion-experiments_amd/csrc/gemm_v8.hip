// ============================================================================ v8
// Weight-stationary GEMM for the short-K, tall-M L1 projections (K = 320, M >= 65536: the
// attention / motion projections and the fused QKV of the 64 x 64 level).  Every other kernel
// restages a W k-tile through LDS per 256-row tile and synchronises the workgroup per k-tile;
// here a workgroup loads ONE 160-column W tile (160 x 320 bf16 = 100 KiB) and its bias into LDS
// once and keeps them, and each of its 8 waves streams 16-row blocks of A straight from global
// memory into MFMA B-operand registers — no A staging, no barrier after the W fill:
//  * per row block a wave runs 10 k-steps x 10 column blocks = 100 MFMAs
//    (v_mfma_f32_16x16x32_bf16); the W fragments are double-buffered in registers (k-step
//    ks + 1's 10 ds_read_b128 go out before k-step ks's MFMAs);
//  * the A registers are double-buffered: the next row block's 10 loads (and this block's
//    residual rows) go out before this block's first MFMA, so each load has a whole row block
//    of MFMA work to land, and the epilogue issues no load (bias from LDS, residual already in
//    registers) — nothing in it waits for the prefetch;
//  * the epilogue stages the wave's 16 x 160 output tile through LDS and writes it back as
//    320-B row segments (1 KiB per store instruction over 3-4 rows) instead of 16 rows x 64 B;
//  * blockIdx % 8 is the XCD; the row blocks are split into 8 contiguous ranges, one per XCD,
//    and inside an XCD each 160-column W tile has 32 / tiles_n workgroups walking the XCD's row
//    blocks in the same order, so an A row block is fetched from HBM once and served from that
//    XCD's L2 to the other column tiles;
//  * the k-order per output (k-steps 0..9, 32 deep each) and the epilogue arithmetic are v2's,
//    so the results equal v2's bits (tests/test_gpu_kernels.py::test_gemm_v8_weight_stationary).
// Measured (tools/kbench.py, 32 images, profiles/r04_gemm_v8.txt): L1 projection 36 vs 52 us,
// with residual 45-50 vs 73-80 us, fused QKV N = 960 125 vs 137 us (v5).  Variants measured
// and not kept: 32-row blocks (4 waves, accumulators in AGPRs: 0.5 W reads per MFMA, slower),
// triple-buffered A, 12 waves per CU, unstaged 64-B stores.
#include "gemm_common.h"

namespace {

constexpr int G8_SUB = G8_BN * BK * 2;  // one 64-deep W sub-tile: 20 KiB

// LNF (round 5, vd_gemm_desc.ln_fold_s): the LayerNorm of A's rows folded in.  Per k-step two
// more MFMAs on the A fragments the wave already holds — ones·x (every output column = the row
// sum) and x·xᵀ (the 16 x 16 Gram block, whose diagonal is the row's sum of squares) — so the
// statistics cost no VALU inside the loop; the epilogue forms rstd·(acc − mean·s[n]) + b'[n]
// with s and b' in LDS next to the bias.  var = E[x²] − mean² in fp32 has a relative error of
// ≈ 1e-7·(1 + mean²/var); where a row's |mean| / std passes 16 (never in the UNet: ≤ 0.1,
// profiles/r06_motion_bisect.txt) the wave takes the exact second pass Σ(x − mean)², re-reading
// its rows from L2 (test_gemm_ln_fold runs rows offset by 30 / 100 / 300 std).
template <bool RES, bool GEGLU, bool PERM = false, bool LNF = false>
__global__ __launch_bounds__(G8_NW * 64, 1) void gemm8_kernel(const vd_gemm_desc d, uint32_t a0_bytes,
                                                             uint32_t w_bytes, uint32_t c_bytes, int tiles_n,
                                                             int groups) {
  constexpr int KS = G8_KMAX / 32, NB = G8_BN / 16, NW = G8_NW;
  constexpr int OROW = G8_BN * 2 + 16;  // staged output row (bytes, padded)
  __shared__ __attribute__((aligned(1024))) char smem[(G8_KMAX / BK) * G8_SUB + G8_BN * 8 + NW * 16 * OROW];
  float* sbias = (float*)(smem + (G8_KMAX / BK) * G8_SUB);
  float* ssum = sbias + G8_BN;  // LNF: s[n] of the tile's columns
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* obuf = smem + (G8_KMAX / BK) * G8_SUB + G8_BN * 8 + wid * 16 * OROW;
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  if (j >= groups * tiles_n) return;  // the XCD's workgroups beyond a whole number of W tiles
  const int nt = j % tiles_n, grp = j / tiles_n;
  const int M = (int)d.M, n0 = nt * G8_BN;
  const int rbs = (M + 15) / 16;
  const int rb0 = (int)((int64_t)rbs * xcd / 8), rb1 = (int)((int64_t)rbs * (xcd + 1) / 8);
  const int gw = grp * NW + wid, GW = groups * NW;

  // ---- W tile -> LDS (5 sub-tiles of 160 rows x 64 k, v2's swizzled B image) + bias, once
  {
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)d.w, 0, w_bytes, 0x00020000);
    const int rb = lane >> 3;
    const uint32_t lc16 = (uint32_t)(((lane & 7) ^ rb) * 16);
    constexpr int PIECES = (G8_KMAX / BK) * (G8_BN / 8);
    for (int p = wid; p < PIECES; p += NW) {
      const int s = p / (G8_BN / 8), pr = p - s * (G8_BN / 8);
      const uint32_t n = (uint32_t)(n0 + pr * 8 + rb);
      dma16(rw, smem + s * G8_SUB + pr * 1024, n * (uint32_t)(d.ldw * 2) + (uint32_t)(s * BK * 2) + lc16);
    }
    if (tid < G8_BN) {
      sbias[tid] = d.bias ? d.bias[n0 + tid] : 0.f;
      if constexpr (LNF) ssum[tid] = d.ln_fold_s[n0 + tid];
    }
    wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  int r = rb0 + gw;
  if (r >= rb1) return;  // no barrier follows
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)d.a0, 0, a0_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void*)d.out, 0, c_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc((void*)(RES ? d.res : d.out), 0, RES ? (uint32_t)(d.M * d.ld_res * 2) : 0u,
                                        0x00020000);
  const int fr = lane & 15, fq = lane >> 4;
  const int wcol = 16 * (fq & 1) + 8 * (fq >> 1);  // lane's column offset inside a swapped pair
  const Rev3 perm = PERM ? Rev3(d.M, d.rmap_n1, d.rmap_n2, d.rmap_inner) : Rev3(0, 0, 0, 0);  // row map
  // this lane's A fragments of row block rb: past the buffer (read as zeros, no traffic) for
  // rows >= M and for row blocks past the XCD's range
  auto load_a = [&](bf16x8 (&x)[KS], int rb) {
    const int m = rb * 16 + fr;
    const uint32_t o = (rb < rb1 && m < M) ? (uint32_t)m * (uint32_t)(d.lda0 * 2) + (uint32_t)(fq * 16) : G2_OOB;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      x[ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ra, o + (uint32_t)(ks * 64), 0, 0));
  };
  u32x4 rsv[NB / 2];
  auto load_res = [&](int rb) {
    const int m = rb * 16 + fr;
#pragma unroll
    for (int pr = 0; pr < NB / 2; ++pr) {
      const uint32_t off = m < M ? (uint32_t)((PERM ? perm(m) : m) * (int)d.ld_res + n0 + pr * 32 + wcol) * 2u : G2_OOB;
      rsv[pr] = __builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, 0);
    }
  };
  const uint32_t wl = 2 * lds_off(fr, fq);  // lane's W fragment byte offset (column block 0, k-step 0)
  auto block = [&](const bf16x8 (&x)[KS], int rb) {
    f32x4 acc[NB];
#pragma unroll
    for (int a = 0; a < NB; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    // k-step ks = sub-tile ks / 2, chunks 4 (ks & 1) + fq: the XOR with (row & 7) is the same
    // for every 16-row column block, so (ks & 1) flips bit 2 of the chunk index (byte bit 6)
    bf16x8 wf[2][NB];
    auto read_w = [&](bf16x8 (&f)[NB], int ks) {
      const char* sb = smem + (ks >> 1) * G8_SUB;
      const uint32_t wk = (ks & 1) ? (wl ^ 64u) : wl;
#pragma unroll
      for (int a = 0; a < NB; ++a) f[a] = *(const bf16x8*)(sb + wk + a * 16 * BK * 2);
    };
    f32x4 sacc = f32x4{0.f, 0.f, 0.f, 0.f}, gacc = f32x4{0.f, 0.f, 0.f, 0.f};  // LNF: ones·x, x·xᵀ
    const bf16x8 ones = __builtin_bit_cast(bf16x8, make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u));
    read_w(wf[0], 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + 1 < KS) read_w(wf[(ks + 1) & 1], ks + 1);
#pragma unroll
      for (int a = 0; a < NB; ++a)
        acc[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks & 1][a], x[ks], acc[a], 0, 0, 0);
      if constexpr (LNF) {
        sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, x[ks], sacc, 0, 0, 0);
        gacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[ks], x[ks], gacc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);  // one k-step per region (unpinned, hipcc spilled)
    }
    // LNF: this lane's outputs all belong to A row rb*16 + fr.  Σx is in every entry of sacc;
    // Σx² is the Gram block's diagonal entry (fr, fr), held by lane fr + 16 (fr >> 2) at index fr & 3
    float nmean = 0.f, rstd = 1.f;
    if constexpr (LNF) {
      const int j3 = fr & 3;
      const float gd = j3 == 0 ? gacc[0] : j3 == 1 ? gacc[1] : j3 == 2 ? gacc[2] : gacc[3];
      const float sxx = __shfl(gd, fr + 16 * (fr >> 2), 64);
      constexpr float RK = 1.0f / (float)G8_KMAX;
      const float mean = sacc[0] * RK;
      float var = fmaf(sxx, RK, -mean * mean);
      if (__any(mean * mean > 256.f * var)) {  // ill-conditioned row(s): exact second pass (see above)
        const int m = rb * 16 + fr;
        const uint32_t o = m < M ? (uint32_t)m * (uint32_t)(d.lda0 * 2) + (uint32_t)(fq * 16) : G2_OOB;
        float ss = 0.f;
#pragma unroll 1
        for (int ks = 0; ks < KS; ++ks) {  // re-read from L2 (the fragments' registers are not kept live)
          const bf16x8 v = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ra, o + (uint32_t)(ks * 64), 0, 0));
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float t = (float)v[e] - mean;
            ss = fmaf(t, t, ss);
          }
        }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        var = ss * RK;
      }
      rstd = rsqrtf(fmaxf(var, 0.f) + d.ln_fold_eps);
      nmean = -mean;
    }
    if constexpr (GEGLU) {
      // (hidden, gate) 16-column block pairs (a, a+1) -> 16 output columns: the lane's 4 outputs
      // (h + bh) * gelu(g + bg) on fp32 pairs (gemm_epilogue's arithmetic), 8 B into the staged row
#pragma unroll
      for (int a = 0; a < NB; a += 2) {
        const int c = a * 16 + 4 * fq;
        const float4 th = *(const float4*)(sbias + c), tg = *(const float4*)(sbias + c + 16);
        const float thv[4] = {th.x, th.y, th.z, th.w}, tgv[4] = {tg.x, tg.y, tg.z, tg.w};
        float hv[4], gv[4];
        if constexpr (LNF) {
          const float4 sh = *(const float4*)(ssum + c), sg = *(const float4*)(ssum + c + 16);
          const float shv[4] = {sh.x, sh.y, sh.z, sh.w}, sgv[4] = {sg.x, sg.y, sg.z, sg.w};
#pragma unroll
          for (int j4 = 0; j4 < 4; ++j4) {
            hv[j4] = fmaf(rstd, fmaf(nmean, shv[j4], acc[a][j4]), thv[j4]);
            gv[j4] = fmaf(rstd, fmaf(nmean, sgv[j4], acc[a + 1][j4]), tgv[j4]);
          }
        } else {
#pragma unroll
          for (int j4 = 0; j4 < 4; ++j4) {
            hv[j4] = acc[a][j4] + thv[j4];
            gv[j4] = acc[a + 1][j4] + tgv[j4];
          }
        }
        uint32_t pk[2];
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          const f32x2 go = gelu_erf2(f32x2{gv[2 * h2], gv[2 * h2 + 1]});
          const f32x2 oo = f32x2{hv[2 * h2], hv[2 * h2 + 1]} * go;
          pk[h2] = pack2(oo[0], oo[1]);
        }
        *(uint2*)(obuf + fr * OROW + ((a / 2) * 16 + 4 * fq) * 2) = make_uint2(pk[0], pk[1]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int it = 0; it < 3; ++it) {  // 16 rows x 160 B
        const int q = it * 64 + lane, row = q / 10, ch = q - row * 10;
        if (q < 160) {
          const uint4 v = *(const uint4*)(obuf + row * OROW + ch * 16);
          const int m = rb * 16 + row;
          const uint32_t off = m < M ? (uint32_t)(m * (int)d.ldc + n0 / 2 + ch * 8) * 2u : G2_OOB;
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{v.x, v.y, v.z, v.w}, rc, off, 0, 0);
        }
      }
      return;
    }
    // epilogue (gemm_epilogue's wide-path arithmetic): permlane16_swap of column blocks (a, a+1)
    // leaves each lane 8 consecutive columns; bias from LDS, residual from rsv
#pragma unroll
    for (int a = 0; a < NB; a += 2) {
      const int c = a * 16 + wcol;
      const float4 t0 = *(const float4*)(sbias + c), t1 = *(const float4*)(sbias + c + 4);
      const float bv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
      float o[8];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        auto rp = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[a][jj]), __float_as_uint(acc[a + 1][jj]),
                                                   false, false);
        o[jj] = __uint_as_float(rp[0]);
        o[4 + jj] = __uint_as_float(rp[1]);
      }
      if constexpr (LNF) {
        const float4 u0 = *(const float4*)(ssum + c), u1 = *(const float4*)(ssum + c + 4);
        const float sv[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) o[jj] = fmaf(rstd, fmaf(nmean, sv[jj], o[jj]), bv[jj]);
      } else {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) o[jj] += bv[jj];
      }
      if (act_is_pw(d.act)) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) o[jj] = act_pw(d.act, o[jj]);
      }
      if constexpr (RES) {
        float rf[8];
        const u32x4 rv = rsv[a / 2];
        unpack8(make_uint4(rv[0], rv[1], rv[2], rv[3]), rf);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) o[jj] += rf[jj];
      }
      *(uint4*)(obuf + fr * OROW + c * 2) = pack8(o);
    }
    // the wave's 16 x 160 tile back out of LDS as 320-B row segments (in-order LDS: no barrier
    // within the wave; out-of-range rows carry an offset past the output buffer, dropped)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < 5; ++it) {
      const int q = it * 64 + lane, row = q / 20, ch = q - row * 20;
      const uint4 v = *(const uint4*)(obuf + row * OROW + ch * 16);
      const int m = rb * 16 + row;
      const uint32_t off = m < M ? (uint32_t)((PERM ? perm(m) : m) * (int)d.ldc + n0 + ch * 8) * 2u : G2_OOB;
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{v.x, v.y, v.z, v.w}, rc, off, 0, 0);
    }
  };
  bf16x8 x0[KS], x1[KS];
  load_a(x0, r);
  for (;;) {
    if constexpr (RES) load_res(r);
    load_a(x1, r + GW);
    block(x0, r);
    if ((r += GW) >= rb1) break;
    if constexpr (RES) load_res(r);
    load_a(x0, r + GW);
    block(x1, r);
    if ((r += GW) >= rb1) break;
  }
}

}  // namespace

namespace vdgemm {

int launch_v8(const vd_gemm_desc& d, const Plan& p, hipStream_t s) {
  const int per_xcd = num_cus() / 8;  // one workgroup per CU, blockIdx % 8 = XCD
  const int tiles_n = (int)(d.N / G8_BN);
  const int groups = per_xcd / tiles_n;
  if (groups < 1) return VD_EINVAL;
  const uint32_t cb = (uint32_t)(d.M * d.ldc * 2);
  const dim3 grid((unsigned)(8 * per_xcd)), block(G8_NW * 64);
  if (d.ln_fold_s && d.act == VD_ACT_GEGLU)
    hipLaunchKernelGGL((gemm8_kernel<false, true, false, true>), grid, block, 0, s, d, p.a0b, p.wb, cb, tiles_n, groups);
  else if (d.ln_fold_s)
    hipLaunchKernelGGL((gemm8_kernel<false, false, false, true>), grid, block, 0, s, d, p.a0b, p.wb, cb, tiles_n, groups);
  else if (d.act == VD_ACT_GEGLU)
    hipLaunchKernelGGL((gemm8_kernel<false, true>), grid, block, 0, s, d, p.a0b, p.wb, cb, tiles_n, groups);
  else if (d.res && d.rmap_inner)
    hipLaunchKernelGGL((gemm8_kernel<true, false, true>), grid, block, 0, s, d, p.a0b, p.wb, cb, tiles_n, groups);
  else if (d.res)
    hipLaunchKernelGGL((gemm8_kernel<true, false>), grid, block, 0, s, d, p.a0b, p.wb, cb, tiles_n, groups);
  else
    hipLaunchKernelGGL((gemm8_kernel<false, false>), grid, block, 0, s, d, p.a0b, p.wb, cb, tiles_n, groups);
  return vd_launch_status();
}

}  // namespace vdgemm
