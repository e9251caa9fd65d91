"""Every HIP entry point with its operands framed by poison and canaries (tests/memframe.py).

The arithmetic tests (test_gpu_kernels.py and its siblings) hand every kernel whole allocations:
what lies behind a row tail is finite debris, the output is the previous case's answer, and no one
looks at the bytes next to it.  Here, for every case:

  1. every tensor input sits in a framed view (0xFF = NaN / -1 all around it),
  2. every caller-supplied output is a framed view left poisoned,
  3. the op runs under poisoned_empty() (its own outputs and workspaces start as 0xFF),
  (a) every frame is intact afterwards — inputs and weights included,
  (b) the output is written everywhere,
  (c) it is within the op's existing tolerance of the fp64 reference its arithmetic test uses,
  (d) with guard rows only (strides as in the plain call) it is bit-identical to the same call
      on ordinary contiguous copies: surrounding memory must not change a bit.

`slack` is the frame's column slack: 0 = guard rows only, 8 = a column-slice view with an aligned
row stride, 2 = a row stride that is no multiple of 8 elements on the operands whose argument
checks allow one (the others keep 8).  Shapes are the smallest that cross each kernel's seams;
a number changed because an argument check refuses the listed one says so where it is set.
"""
import contextlib
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import memframe as mf
from memframe import close_bf16, close_f32
from vdiff import ops
from vdiff._lib import check, lib

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
LOG2E = math.log2(math.e)
SLACKS = (0, 8, 2)

# Entry point -> the framed tests that launch it, or why it launches nothing
# (tests/test_memframe_host.py pins the keys to vdiff._lib.SIGNATURES).
COVERAGE = {
    "vd_strerror": "no launch: returns a static string",
    "vd_version": "no launch: returns a constant",
    "vd_build_hash": "no launch: returns a static string",
    "vd_build_arch": "no launch: returns a static string",
    "vd_gemm": ("test_gemm_v1", "test_gemm_v9", "test_gemm_v2", "test_gemm_v2_splitk", "test_gemm_v2_narrow_n",
                "test_gemm_v3", "test_gemm_v5", "test_gemm_ln_fused_epilogue", "test_gemm_v6", "test_gemm_v6_splitk",
                "test_gemm_v8", "test_conv3x3", "test_conv3d"),
    "vd_gemm_ws_bytes": "no launch: a size query (its answer is the exact size of the framed split-K workspaces)",
    "vd_gemm_plan": "no launch: a plan query (every GEMM case asserts its answer)",
    "vd_ff_fused": ("test_ff_fused",),
    "vd_ff_fused_takes": "no launch: a shape query",
    "vd_gn_partial": ("test_group_norm_four_launch",),
    "vd_gn_finalize": ("test_group_norm_four_launch",),
    "vd_gn_finalize_g": ("test_group_norm_four_launch",),
    "vd_gn_finalize_g_ranks": ("test_group_norm_four_launch",),
    "vd_gn_small": ("test_gn_small",),
    "vd_gn_apply": ("test_group_norm_four_launch",),
    "vd_gn_apply_rev3": ("test_group_norm_four_launch",),
    "vd_gn_partial_g": ("test_group_norm_2pass", "test_group_norm_four_launch"),
    "vd_gn_apply_g": ("test_group_norm_2pass",),
    "vd_layernorm": ("test_layer_norm",),
    "vd_attention": ("test_attention_abi_entry_points",),
    "vd_attention_f32": ("test_attention_abi_entry_points",),
    "vd_attention_ex": ("test_attention", "test_attention_flash40_fixup"),
    "vd_attention_plan": "no launch: a plan query",
    "vd_temporal_attention": ("test_temporal_attention",),
    "vd_temporal_attention_valu": ("test_temporal_attention",),
    "vd_temporal_attention_kv": ("test_temporal_attention_kv",),
    "vd_motion_qkv_attention": ("test_motion_qkv_attention",),
    "vd_motion_qkv_attention_takes": "no launch: a shape query",
    "vd_temporal_attention_rope": ("test_temporal_attention_rope",),
    "vd_softmax_rows": ("test_softmax_rows",),
    "vd_frame_metrics": ("test_frame_sums",),
    "vd_farneback_workspace": "no launch: a size query (its answer is the exact size of the framed workspace)",
    "vd_farneback_flow": ("test_farneback_flow_and_sums",),
    "vd_flow_warp_workspace": "no launch: a size query (its answer is the exact size of the framed workspace)",
    "vd_flow_warp_stats": ("test_farneback_flow_and_sums",),
    "vd_conv2d_f32": ("test_conv2d_f32",),
    "vd_lpips_layer_workspace": "no launch: a size query (its answer is the exact size of the framed workspace)",
    "vd_lpips_layer": ("test_lpips_layer",),
    "vd_lpips_workspace": "no launch: a size query (its answer is the exact size of the framed workspace)",
    "vd_lpips_pairs": ("test_lpips_pairs",),
    "vd_timestep_embed": ("test_timestep_embed",),
    "vd_pack_latents": ("test_pack_unpack",),
    "vd_unpack_nhwc": ("test_pack_unpack",),
    "vd_ddim_cfg_step": ("test_cfg_step",),
    "vd_euler_cfg_step": ("test_cfg_step",),
    "vd_step_advance": ("test_step_advance",),
    "vd_block_transpose": ("test_block_transpose",),
    "vd_patchify": ("test_patchify_unpatchify",),
    "vd_unpatchify": ("test_patchify_unpatchify",),
    "vd_rope_qk": ("test_rope_qk",),
    "vd_attention_fp8_quant": ("test_attention_fp8",),
    "vd_attention_fp8_quant_rope": ("test_attention_fp8",),
    "vd_attention_fp8": ("test_attention_fp8",),
    "vd_rows_eltwise": ("test_rows_add", "test_silu_rows"),
    "vd_upsample_nearest2x": ("test_upsample2x_rows",),
    "vd_res_ln_mod": ("test_res_ln_mod",),
}


# ---------------------------------------------------------------- the procedure
class Mk:
    """Operand maker of one run.  slack = None: plain contiguous tensors (the ordinary call of
    check (d)); else framed views with that column slack, all of them remembered for check (a),
    the outputs for check (b)."""

    def __init__(self, slack, dev="cuda"):
        self.slack, self.dev, self.frames, self.outs = slack, dev, [], []

    @property
    def framed(self):
        return self.slack is not None

    def _slack(self, slack, unaligned):
        s = self.slack if slack is None else slack
        return s if s % 8 == 0 or unaligned else 8

    def rows(self, t, name="", slack=None, unaligned=False):
        """A 2-D row operand holding t.  unaligned: its row stride need not be a multiple of 8."""
        if not self.framed:
            return t.contiguous().clone()
        v, f = mf.load2d(t, col_slack=self._slack(slack, unaligned), name=name)
        self.frames.append(f)
        return v

    def flat(self, t, name=""):
        """A contiguous operand of any shape holding t (vectors, weight blobs, latents)."""
        if t is None:
            return None
        if not self.framed:
            return t.contiguous().clone()
        v, f = mf.loadnd(t, name=name)
        self.frames.append(f)
        return v

    def out(self, shape, dtype=BF, name="out", slack=None, unaligned=True):
        """A caller-supplied 2-D output, poisoned."""
        if not self.framed:
            return torch.empty(shape, device=self.dev, dtype=dtype)
        v, f = mf.framed(shape, dtype, self.dev, col_slack=self._slack(slack, unaligned), name=name)
        self.frames.append(f)
        self.outs.append(f)
        return v

    def out_flat(self, shape, dtype, name="out"):
        if not self.framed:
            return torch.empty(shape, device=self.dev, dtype=dtype)
        v, f = mf.framed_nd(shape, dtype, self.dev, name=name)
        self.frames.append(f)
        self.outs.append(f)
        return v

    def ws(self, nbytes, name="workspace"):
        """A workspace of exactly nbytes bytes (the size the library advertises), poisoned."""
        v, f = mf.framed_1d(max(int(nbytes), 0), torch.uint8, self.dev, name=name)
        self.frames.append(f)
        return v


def run(fn, slack=0, bitwise=True):
    """Steps 1-3 and checks (a), (b), (d) for fn(mk) -> output tensor(s); returns the framed
    run's outputs for check (c)."""
    mk = Mk(slack)
    with mf.poisoned_empty():
        got = fn(mk)
    torch.cuda.synchronize()
    got = got if isinstance(got, tuple) else (got,)
    for f in mk.frames:
        f.assert_intact()                                   # (a)
    for f in mk.outs:
        f.assert_written()                                  # (b) caller-supplied outputs
    for i, t in enumerate(got):
        mf.assert_no_poison(t, f"output {i}")               # (b) outputs the wrapper allocated
    if slack == 0 and bitwise:                              # (d)
        plain = fn(Mk(None))
        torch.cuda.synchronize()
        plain = plain if isinstance(plain, tuple) else (plain,)
        for i, (a, b) in enumerate(zip(got, plain)):
            same = torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
            assert same, (f"output {i} depends on the memory around the operands: "
                          f"{int((a != b).sum())} of {a.numel()} elements differ from the plain call")
    return got


def rnd(*shape, std=1.0, g=None):
    return (torch.randn(*shape, device="cuda", generator=g) * std).to(BF)


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---------------------------------------------------------------- GEMM
@contextlib.contextmanager
def gemm_launches(mk=None):
    """Inside the block every vd_gemm of vdiff.ops reports the plan (kernel, split) of the very
    descriptor it launches, and — with mk — runs on a framed split-K workspace of exactly
    vd_gemm_ws_bytes bytes through lib().vd_gemm (for v6 that includes the arrival counters)
    instead of the wrapper's own torch.empty one."""
    plans, orig = [], ops._run_gemm

    def run_gemm(d, device, what):
        plans.append(ops.gemm_plan_of(d))
        if mk is None or not mk.framed:
            return orig(d, device, what)
        nbytes = lib().vd_gemm_ws_bytes(C.byref(d))
        if nbytes > 0:
            ws = mk.ws(nbytes, "split-K workspace")
            d.ws, d.ws_bytes = ws.data_ptr(), nbytes
        check(lib().vd_gemm(C.byref(d), torch.cuda.current_stream().cuda_stream), what)

    ops._run_gemm = run_gemm
    try:
        yield plans
    finally:
        ops._run_gemm = orig


def geglu_ref(y):
    h, g = y.chunk(2, -1)
    return h * F.gelu(g)


def epilogue_ref(y, epi):
    if epi == "silu":
        return F.silu(y)
    if epi == "gelu":
        return F.gelu(y)
    if epi == "geglu":
        return geglu_ref(y)
    return y


def gemm_case(slack, M, N, K, *, path, want_plan, k0=None, epi="bias", res=False, rowbias=False, rmap=None,
              ln_fold=False, mul=1, seed=0, f32_rtol=1e-3):
    """One framed ops.gemm against fp64.  epi: bias | nobias | silu | gelu | geglu (N = the packed
    width, output N / 2) | f32 (out_f32).  want_plan: (kernel, split), split None = at least 2.
    Odd slacks give `res` / `out` / `rowbias` a row stride that is no multiple of 8 (A, W: ld % 8)."""
    from vdiff.models.layers import LnFold, pack_geglu
    g = gen(seed + M + N + K)
    k0 = K if k0 is None else k0
    a = rnd(M, k0, g=g)
    a1 = rnd(M, K - k0, g=g) if k0 < K else None
    w = rnd(N, K, std=K ** -0.5, g=g)
    b = None if epi == "nobias" else torch.randn(N, device="cuda", generator=g)
    geglu, out_f32 = epi == "geglu", epi == "f32"
    act = {"silu": ops.ACT_SILU, "gelu": ops.ACT_GELU, "geglu": ops.ACT_GEGLU}.get(epi, ops.ACT_NONE)
    r = rnd(M, N, g=g) if res else None
    rb_rows, rb_div = 3, -(-M // 3)
    rb = torch.randn(rb_rows, N, device="cuda", generator=g) if rowbias else None
    x = a if a1 is None else torch.cat([a, a1], 1)
    if ln_fold:
        a = x = (1.7 * (a.float() + 0.5 * torch.randn(M, 1, device="cuda", generator=g))).to(BF)
        norm = torch.nn.LayerNorm(K).to("cuda")
        with torch.no_grad():
            norm.weight.copy_(1 + 0.2 * torch.randn(K, device="cuda", generator=g))
            norm.bias.copy_(0.1 * torch.randn(K, device="cuda", generator=g))
        fold = LnFold(norm, w.float(), b, pack=pack_geglu if geglu else None)
        wk, bk, sk = fold.w, fold.b, fold.s
        xd = x.double()
        mean, rstd = xd.mean(1, keepdim=True), (xd.var(1, unbiased=False, keepdim=True) + fold.eps).rsqrt()
        y = rstd * (xd @ wk.double().T - mean * sk.double()) + bk.double()
        if geglu:  # packed: (hidden block i, gate block i) 16-column pairs
            y = y.reshape(M, -1, 2, 16)
            want = y[:, :, 0].reshape(M, -1) * F.gelu(y[:, :, 1].reshape(M, -1))
        else:
            want = y
    else:
        wk, bk, sk = (pack_geglu(w), pack_geglu(b) if b is not None else None, None) if geglu else (w, b, None)
        y = x.double() @ w.double().T + (b.double() if b is not None else 0)
        if rb is not None:
            y = y + rb.double()[torch.arange(M, device="cuda") // rb_div]
        want = epilogue_ref(y, epi)
        if rmap is not None:
            from vdiff.dist import rev3_reference
            want = rev3_reference(want, *rmap)
        if r is not None:
            want = want + r.double()
    n_out = N // 2 if geglu else N
    plans = []

    def fn(mk):
        kw = {}
        if r is not None:
            kw["res"] = mk.rows(r, "res", unaligned=True)
        if rb is not None:
            kw["rowbias"], kw["rb_div"] = mk.rows(rb, "rowbias", unaligned=True), rb_div
        if rmap is not None:
            kw["rmap"] = rmap
        if sk is not None:
            kw["ln_fold"] = (mk.flat(sk, "ln_fold s"), fold.eps)
        out = mk.out((M, n_out), F32 if out_f32 else BF)
        with ops.gemm_plan(path=path), ops.plan_scaled(mul), gemm_launches(mk if mk.slack != 8 else None) as p:
            ops.gemm(mk.rows(a, "a"), mk.rows(wk, "w"), a1=mk.rows(a1, "a1") if a1 is not None else None,
                     bias=mk.flat(bk, "bias"), act=act, out=out, out_f32=out_f32, **kw)
        plans.append(p)
        return out

    (got,) = run(fn, slack)
    for p in plans:
        assert len(p) == 1 and p[0][0] == want_plan[0], f"planned {p}, the case is for kernel v{want_plan[0]}"
        assert p[0][1] == want_plan[1] if want_plan[1] else p[0][1] >= 2, f"planned split {p[0][1]}"
    if out_f32:
        close_f32(got, want, rtol=f32_rtol, atol=1e-3 if want_plan[1] != 1 else 1e-4)
    else:
        close_bf16(got, want)


EPIS = ("bias", "nobias", "silu", "gelu", "f32")


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("M,N,K,k0,epi,res", [(130, 100, 96, 64, "bias", True), (130, 100, 96, 64, "silu", False),
                                              (130, 100, 96, 64, "f32", False), (130, 128, 96, 64, "geglu", False),
                                              (40, 72, 64, 64, "gelu", False), (40, 72, 64, 64, "nobias", True)])
def test_gemm_v1(cuda, slack, M, N, K, k0, epi, res):
    """v1: two row tiles with a ragged edge, the a0 | a1 concat, N % 8 == 4; M = 40 is below every
    other kernel's floor (the automatic plan).  GEGLU needs N % 32 == 0: 128 for the listed 100."""
    gemm_case(slack, M, N, K, path=1 if M > 64 else 0, want_plan=(1, 1), k0=k0, epi=epi, res=res, rowbias=res)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("epi,res", [("bias", True), ("silu", False), ("gelu", False), ("f32", False), ("nobias", False)])
def test_gemm_v9(cuda, slack, epi, res):
    """v9 (M <= 16): a partial last 16-column block (N = 136); fp32 output at its own test's rtol 1e-4."""
    gemm_case(slack, 3, 136, 320, path=9, want_plan=(9, 1), epi=epi, res=res, rowbias=res, f32_rtol=1e-4)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("epi,res", [("bias", True), ("silu", False), ("gelu", False), ("f32", False), ("geglu", False)])
def test_gemm_v2(cuda, slack, epi, res):
    """v2 (256-row LDS-DMA tiles, buffer-resource range checks): a ragged second row tile, a
    partial last column tile (N = 328; 320 under GEGLU, which needs N % 32 == 0), a0 | a1, a
    column-slice row bias, residual and output as slack-column views."""
    gemm_case(slack, 300, 320 if epi == "geglu" else 328, 128, path=2, want_plan=(2, 1), k0=64, epi=epi, res=res,
              rowbias=res)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("epi,res", [("bias", True), ("silu", False), ("gelu", False), ("f32", False), ("geglu", False)])
def test_gemm_v2_splitk(cuda, slack, epi, res):
    """gemm_splitk.hip: fp32 slabs in a poisoned workspace of exactly the advertised size, every
    element of which the reduce then reads."""
    gemm_case(slack, 300, 160, 1024, path=2, want_plan=(2, None), epi=epi, res=res, rowbias=res)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("N", [4, 24])
@pytest.mark.parametrize("epi", ["bias", "f32"])
def test_gemm_v2_narrow_n(cuda, slack, N, epi):
    gemm_case(slack, 264, N, 64, path=0, want_plan=(2, 1), epi=epi)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("N,epi,res", [(264, "bias", True), (264, "silu", False), (264, "gelu", False),
                                       (264, "f32", False), (288, "geglu", False)])
def test_gemm_v3(cuda, slack, N, epi, res):
    """v3 (256 x 256): ragged in M and N.  GEGLU needs N % 32 == 0: 288 for the listed 264."""
    gemm_case(slack, 300, N, 64, path=3, want_plan=(3, 1), epi=epi, res=res)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("epi,res", [("bias", True), ("nobias", False), ("silu", False), ("gelu", False), ("f32", False),
                                     ("geglu", False)])
def test_gemm_v5(cuda, slack, epi, res):
    """v5: the load-free epilogue's unconditional buffer stores at a ragged M and N (N = 328; 320
    under GEGLU), k0 = 64 of K = 96."""
    gemm_case(slack, 300, 320 if epi == "geglu" else 328, 96, path=5, want_plan=(5, 1), k0=64, epi=epi, res=res)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("epi,res,rmap,ln_fold", [("bias", True, None, False), ("silu", False, None, False),
                                                  ("gelu", False, None, False), ("geglu", False, None, False),
                                                  ("f32", False, None, False), ("bias", True, (2, 2, 1), False),
                                                  ("bias", False, None, True)])
def test_gemm_v6(cuda, slack, epi, res, rmap, ln_fold):
    """v6 unsplit (M < 256: the automatic plan): two ragged 64-row tiles, N = 136; with the row
    map (M = 100 = 25 x 2 x 2 x 1) and with a folded LayerNorm.  GEGLU needs N % 32 == 0: 128."""
    gemm_case(slack, 100, 128 if epi == "geglu" else 136, 64, path=0, want_plan=(6, 1), epi=epi, res=res, rmap=rmap,
              ln_fold=ln_fold, rowbias=res and rmap is None)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("epi,res", [("bias", True), ("silu", False), ("gelu", False), ("f32", False), ("geglu", False)])
def test_gemm_v6_splitk(cuda, slack, epi, res):
    """v6's in-kernel split-K reduce: slabs AND arrival counters in a poisoned workspace of exactly
    the advertised size.  The plan splits v6 from 256 planned rows only, so the 100 launched rows
    are planned as 300 (plan_scaled), as a frame shard's chunk is."""
    gemm_case(slack, 100, 320, 2560, path=6, want_plan=(6, None), epi=epi, res=res, rowbias=res, mul=3)


@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("N,epi,res,rmap,ln_fold", [(320, "bias", False, None, False), (960, "nobias", False, None, False),
                                                    (320, "bias", True, None, False), (960, "silu", False, None, False),
                                                    (320, "gelu", False, None, False),
                                                    (320, "bias", True, (2, 2, 1), False),
                                                    (2560, "geglu", False, None, False),
                                                    (960, "bias", False, None, True),
                                                    (2560, "geglu", False, None, True)])
def test_gemm_v8(cuda, slack, N, epi, res, rmap, ln_fold):
    """v8 (weight-stationary, K = 320): M = 4096 + 37, a partial last 32-row block.  The row map
    needs M % (n1 n2 inner) == 0: 4096 + 36 there.  v8 takes ldc % 8 == 0 only (the plan leaves
    it otherwise), so there is no unaligned-stride variant."""
    M = 4096 + (36 if rmap else 37)
    gemm_case(slack, M, N, 320, path=8, want_plan=(8, 1), epi=epi, res=res, rmap=rmap, ln_fold=ln_fold)


@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("res,pe", [(True, False), (False, True), (True, True)])
def test_gemm_ln_fused_epilogue(cuda, slack, res, pe):
    """gemm_ln on v5's fused LayerNorm epilogue (one 256 x 320 tile owns whole rows): 300 rows
    planned as 110 x 300 (>= 128 row tiles).  out and ln_out both framed."""
    M, N, K, frames, pos, mul = 300, 320, 64, 16, 7, 110
    assert (M * mul + 255) // 256 >= 128
    g = gen(5)
    a, w = rnd(M, K, g=g), rnd(N, K, std=K ** -0.5, g=g)
    b = torch.randn(N, device=cuda, generator=g) * 0.1
    r = rnd(M, N, g=g) if res else None
    gam = 1 + 0.1 * torch.randn(N, device=cuda, generator=g)
    bet = 0.1 * torch.randn(N, device=cuda, generator=g)
    pet = torch.randn(32, N, device=cuda, generator=g) if pe else None
    plans = []

    def fn(mk):
        kw = dict(pe=mk.flat(pet, "pe"), pe_div=pos, pe_period=frames) if pe else {}
        out, ln = mk.out((M, N), name="out", unaligned=False), mk.out((M, N), name="ln_out", unaligned=False)
        with ops.gemm_plan(path=5), ops.plan_scaled(mul), gemm_launches(mk) as p:
            ops.gemm_ln(mk.rows(a, "a"), mk.rows(w, "w"), mk.flat(gam, "gamma"), mk.flat(bet, "beta"),
                        bias=mk.flat(b, "bias"), res=mk.rows(r, "res") if res else None, out=out, ln_out=ln, **kw)
        plans.append(p)
        return out, ln

    out, ln = run(fn, slack)
    assert all(p == [(5, 1)] for p in plans), plans
    want = a.double() @ w.double().T + b.double() + (r.double() if res else 0)
    close_bf16(out, want)
    ref = F.layer_norm(out.double(), (N,), gam.double(), bet.double(), eps=1e-5)
    if pe:
        ref = ref + pet.double()[(torch.arange(M, device=cuda) // pos) % frames]
    close_bf16(ln, ref)


# ---------------------------------------------------------------- conv3x3 / conv3d
def conv_case(slack, n, h, w, c0, c1, co, *, stride=1, up=False, path=0, want_ver, out_f32=True, res=False, seed=0,
              want_split=1):
    from vdiff.models.layers import pack_conv3x3
    g = gen(seed + c0 + co + h)
    x0 = rnd(n * h * w, c0, g=g)
    x1 = rnd(n * h * w, c1, g=g) if c1 else None
    wt = (torch.randn(co, c0 + c1, 3, 3, device="cuda", generator=g) * (9 * (c0 + c1)) ** -0.5).to(BF)
    b = torch.randn(co, device="cuda", generator=g)
    wp = pack_conv3x3(wt)
    ho, wo = (2 * h, 2 * w) if up else ((h - 1) // stride + 1, (w - 1) // stride + 1)
    r = rnd(n * ho * wo, co, g=g) if res else None
    plans = []

    def fn(mk):
        out = mk.out((n * ho * wo, co), F32 if out_f32 else BF)
        with ops.gemm_plan(path=path), gemm_launches(mk if mk.slack != 8 else None) as p:
            ops.conv3x3(mk.rows(x0, "x0"), n, h, w, mk.rows(wp, "w"), x1=mk.rows(x1, "x1") if c1 else None,
                        stride=stride, upsample=up, bias=mk.flat(b, "bias"),
                        res=mk.rows(r, "res", unaligned=True) if res else None, out=out, out_f32=out_f32)
        plans.append(p)
        return out

    (got,) = run(fn, slack)
    for p in plans:
        assert len(p) == 1 and p[0][0] == want_ver and (p[0][1] == 1 if want_split == 1 else p[0][1] >= 2), p
    xin = x0 if x1 is None else torch.cat([x0, x1], 1)
    img = xin.double().reshape(n, h, w, -1).permute(0, 3, 1, 2)
    if up:
        img = F.interpolate(img, scale_factor=2.0, mode="nearest")
    want = F.conv2d(img.cpu(), wt.double().cpu(), b.double().cpu(), stride=stride, padding=1)
    want = want.permute(0, 2, 3, 1).reshape(-1, co)
    if res:
        want = want + r.double().cpu()
    if out_f32:
        close_f32(got, want, rtol=1e-3, atol=(1e-3 if want_split != 1 else 1e-4) * max(1.0, want.abs().max().item()))
    else:
        close_bf16(got, want)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("case", ["s1", "s2", "up", "concat", "cout4", "v6split"])
def test_conv3x3(cuda, slack, case):
    """2 images of 9 x 7 (126 output rows on v6's 64-row tiles, 504 upsampled; the taps past image
    0's border abut image 1, those of image 1 the frame; stride 2 leaves 40 rows and the 32 + 32
    concat a k0 that is no multiple of 64: both v1), Cout 72; Cout 4 on 2 images of
    12 x 11 (264 rows: the 256 x 32 v2 tile); the split-K v6 conv at M < 256 rows is planned as
    its 4-fold row count (v6 splits from 256 planned rows)."""
    if case == "cout4":
        return conv_case(slack, 2, 12, 11, 64, 0, 4, want_ver=2, res=False)
    if case == "v6split":
        return conv_case_v6_split(slack)
    c1 = 32 if case == "concat" else 0
    conv_case(slack, 2, 9, 7, 32 if c1 else 64, c1, 72, stride=2 if case == "s2" else 1, up=case == "up",
              want_ver=1 if case in ("s2", "concat") else 6, res=case == "s1", out_f32=case != "s1")


def conv_case_v6_split(slack):
    from vdiff.models.layers import pack_conv3x3
    n, h, w, ci, co = 2, 9, 7, 640, 128
    g = gen(77)
    x0 = rnd(n * h * w, ci, g=g)
    wt = (torch.randn(co, ci, 3, 3, device="cuda", generator=g) * (9 * ci) ** -0.5).to(BF)
    b = torch.randn(co, device="cuda", generator=g)
    wp = pack_conv3x3(wt)
    plans = []

    def fn(mk):
        out = mk.out((n * h * w, co), BF)
        with ops.gemm_plan(path=6), ops.plan_scaled(4), gemm_launches(mk if mk.slack != 8 else None) as p:
            ops.conv3x3(mk.rows(x0, "x0"), n, h, w, mk.rows(wp, "w"), bias=mk.flat(b, "bias"), out=out)
        plans.append(p)
        return out

    (got,) = run(fn, slack)
    assert all(len(p) == 1 and p[0][0] == 6 and p[0][1] >= 2 for p in plans), plans
    img = x0.double().reshape(n, h, w, -1).permute(0, 3, 1, 2)
    want = F.conv2d(img.cpu(), wt.double().cpu(), b.double().cpu(), padding=1).permute(0, 2, 3, 1).reshape(-1, co)
    close_bf16(got, want)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("ks", [3, 1])
@pytest.mark.parametrize("halo", [False, True])
def test_conv3d(cuda, slack, ks, halo):
    """conv3d kt 3 x ks {3, 1}: batch 2, 3 frames of 6 x 5 — the temporal taps of video 0's last
    frame must stop at its end, not read video 1; the halo form reads frames_out + 2 frames."""
    from vdiff.models.layers import pack_conv3d
    B, T, h, w, ci, co = 2, 3, 6, 5, 64, 72
    g = gen(31 + ks)
    Tin = T + 2 if halo else T
    x = rnd(B * Tin * h * w, ci, g=g)
    wt = (torch.randn(co, ci, 3, ks, ks, device=cuda, generator=g) * 0.05).to(BF)
    b = torch.randn(co, device=cuda, generator=g)
    wp = pack_conv3d(wt)
    plans = []

    def fn(mk):
        out = mk.out((B * T * h * w, co), F32)
        with gemm_launches(mk) as p:
            ops.conv3d(mk.rows(x, "x"), B, Tin, h, w, mk.rows(wp, "w"), kt=3, ks=ks, frames_out=T, t_off=1 if halo else 0,
                       bias=mk.flat(b, "bias"), out=out, out_f32=True)
        plans.append(p)
        return out

    (got,) = run(fn, slack)
    assert all(p == [(1, 1)] for p in plans), plans  # temporal taps below 256 rows: v1
    vid = x.double().reshape(B, Tin, h, w, ci).permute(0, 4, 1, 2, 3).cpu()
    want = F.conv3d(vid, wt.double().cpu(), b.double().cpu(), padding=(0 if halo else 1, ks // 2, ks // 2))
    want = want.permute(0, 2, 3, 4, 1).reshape(-1, co)
    close_f32(got, want, rtol=1e-3, atol=1e-4 * max(1.0, want.abs().max().item()))


# ---------------------------------------------------------------- ff_fused
@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("M", [16, 300])
def test_ff_fused(cuda, slack, folded, M):
    """vd_ff_fused: x, res and out as slack-column views, out poisoned; against fp64 (LayerNorm ->)
    Linear -> GEGLU -> Linear + residual at the bound of tests/test_gpu_ff_fused.py."""
    from vdiff.models.layers import LnFold, pack_geglu
    Cc, HID = 320, 1280
    g = gen(1234 + M)
    x, r = rnd(M, Cc, g=g), rnd(M, Cc, g=g)
    w1 = 0.02 * torch.randn(2 * HID, Cc, device=cuda, generator=g)
    b1 = 0.02 * torch.randn(2 * HID, device=cuda, generator=g)
    w2 = (0.02 * torch.randn(Cc, HID, device=cuda, generator=g)).to(BF)
    b2 = 0.02 * torch.randn(Cc, device=cuda, generator=g)
    norm = torch.nn.LayerNorm(Cc).to(cuda)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(Cc, device=cuda, generator=g))
        norm.bias.copy_(0.1 * torch.randn(Cc, device=cuda, generator=g))
    if folded:
        fold = LnFold(norm, w1, b1, pack=pack_geglu)
        w1k, b1k, s = fold.w, fold.b, fold.s
    else:
        w1k, b1k, s = pack_geglu(w1.to(BF)), pack_geglu(b1), None

    def fn(mk):
        out = mk.out((M, Cc), unaligned=False)
        ops.ff_fused(mk.rows(x, "x"), mk.flat(w1k, "w1"), mk.flat(w2, "w2"), b1=mk.flat(b1k, "b1"), b2=mk.flat(b2, "b2"),
                     res=mk.rows(r, "res"), ln_fold=(mk.flat(s, "s"), fold.eps) if folded else None, out=out)
        return out

    (got,) = run(fn, slack)
    xd = x.double()
    if folded:
        xd = F.layer_norm(xd, (Cc,), norm.weight.double(), norm.bias.double(), norm.eps)
    y = xd @ (w1.double() if folded else w1.to(BF).double()).T + b1.double()
    ref = (y[:, :HID] * F.gelu(y[:, HID:])) @ w2.double().T + b2.double() + r.double()
    e = got.double() - ref
    assert (e.norm() / ref.norm()).item() < 2 ** -8 and e.abs().max().item() < 2 ** -7 * ref.abs().max().item()


# ---------------------------------------------------------------- norms
def gn_ref(x, n, pix, C, G, gamma, beta, eps, silu):
    t = x.double().reshape(n, pix, C).permute(0, 2, 1)
    want = F.group_norm(t, G, gamma.double(), beta.double(), eps)
    return (F.silu(want) if silu else want).permute(0, 2, 1).reshape(-1, C)


def gn_data(n, pix, c0, c1, seed):
    g = gen(seed)
    x0 = (rnd(n * pix, c0, g=g).float() * 3 + 1.5).to(BF)
    x1 = (rnd(n * pix, c1, g=g).float() - 0.7).to(BF)
    gamma = torch.rand(c0 + c1, device="cuda", generator=g) + 0.5
    beta = torch.randn(c0 + c1, device="cuda", generator=g)
    return x0, x1, gamma, beta


@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("C,rows_pe", [(320, False), (640, True), (1280, False), (64, True), (128, False),
                                       (1152, True), (2048, False), (320, True), (2048, True)])
def test_layer_norm(cuda, slack, C, rows_pe):
    """vd_layernorm: several rows per wave (C 320 / 640 / 1280) and one row per wave (the rest), 77
    rows — the last wave's rows past 77 are the frame — with and without the PE by frame."""
    rows = 77
    g = gen(C)
    x = (rnd(rows, C, g=g).float() * 2 + 0.3).to(BF)
    gam, bet = torch.rand(C, device=cuda, generator=g) + 0.5, torch.randn(C, device=cuda, generator=g)
    pe = torch.randn(16, C, device=cuda, generator=g) if rows_pe else None

    def fn(mk):
        kw = dict(pe=mk.flat(pe, "pe"), pe_div=3, pe_period=16) if rows_pe else {}
        out = mk.out((rows, C), unaligned=False)
        ops.layer_norm(mk.rows(x, "x"), mk.flat(gam, "gamma"), mk.flat(bet, "beta"), out=out, **kw)
        return out

    (got,) = run(fn, slack)
    ref = F.layer_norm(x.double(), (C,), gam.double(), bet.double(), 1e-5)
    if rows_pe:
        ref = ref + pe.double()[(torch.arange(rows, device=cuda) // 3) % 16]
    close_bf16(got, ref)


@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("silu", [True, False])
def test_gn_small(cuda, slack, silu):
    """vd_gn_small: n 2, pix 64, C 256 as the 128 + 128 concat."""
    n, pix, C, G, eps = 2, 64, 256, 32, 1e-5
    assert ops.gn_small_chunk(pix, C, G)
    x0, x1, gam, bet = gn_data(n, pix, 128, 128, 3)

    def fn(mk):
        out = mk.out((n * pix, C), unaligned=False)
        return ops.gn_small(mk.rows(x0, "x0"), n, pix, G, eps, mk.flat(gam, "gamma"), mk.flat(bet, "beta"), silu=silu,
                            x1=mk.rows(x1, "x1"), out=out)

    (got,) = run(fn, slack)
    close_bf16(got, gn_ref(torch.cat([x0, x1], 1), n, pix, C, G, gam, bet, eps, silu))


@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("own_records", [False, True])
def test_group_norm_2pass(cuda, slack, own_records):
    """vd_gn_partial_g + vd_gn_apply_g: n 2, pix 100 (ragged splits and row blocks), C 320 as
    192 + 128; the records from the wrapper's poisoned torch.empty, or (own_records) in a framed
    buffer of exactly n x splits x groups float4 through lib()."""
    n, pix, C, G, eps = 2, 100, 320, 32, 1e-6
    x0, x1, gam, bet = gn_data(n, pix, 192, 128, 4)
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def fn(mk):
        a0, a1, gm, bt = mk.rows(x0, "x0"), mk.rows(x1, "x1"), mk.flat(gam, "gamma"), mk.flat(bet, "beta")
        out = mk.out((n * pix, C), unaligned=False)
        if not (own_records and mk.framed):
            return ops.group_norm_2pass(a0, n, pix, G, eps, gm, bt, silu=True, x1=a1, out=out)
        ns = ops.gn_image_splits(pix)
        ws = mk.ws(n * ns * G * 16, "records")
        check(lib().vd_gn_partial_g(a0.data_ptr(), a0.stride(0), 192, a1.data_ptr(), a1.stride(0), C, n, pix, ns, G,
                                    ws.data_ptr(), st()), "vd_gn_partial_g")
        rpb = math.ceil(pix / ops.gn_apply_blocks(n, pix, C))
        check(lib().vd_gn_apply_g(a0.data_ptr(), a0.stride(0), 192, a1.data_ptr(), a1.stride(0), C, n, pix,
                                  ws.data_ptr(), ns, G, eps, gm.data_ptr(), bt.data_ptr(), 1, out.data_ptr(),
                                  out.stride(0), rpb, st()), "vd_gn_apply_g")
        return out

    (got,) = run(fn, slack)
    close_bf16(got, gn_ref(torch.cat([x0, x1], 1), n, pix, C, G, gam, bet, eps, True))


@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("kind", ["group", "channel", "ranks", "wrapper"])
def test_group_norm_four_launch(cuda, slack, kind):
    """The partial / finalize / apply path (two_pass=False) with its record and scale / shift
    buffers framed at exactly their size through lib(): per-group records + the rev3 apply,
    per-channel records + the plain apply, the rank-major finalize over two pixel halves; and once
    through ops.group_norm with the wrapper's own poisoned buffers."""
    from vdiff.dist import rev3_reference
    n, pix, C, c0, G, eps = 2, 100, 320, 192, 32, 1e-6
    x0, x1, gam, bet = gn_data(n, pix, c0, C - c0, 6)
    ns = ops.gn_splits(n, pix)
    rev3 = (2, 2, 2) if kind == "group" else None
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    L = lib()

    def fn(mk):
        a0, a1, gm, bt = mk.rows(x0, "x0"), mk.rows(x1, "x1"), mk.flat(gam, "gamma"), mk.flat(bet, "beta")
        if kind == "wrapper" or not mk.framed:
            if kind == "ranks":  # the plain call of check (d): the same records in instance-major order
                return ops.group_norm(a0, n, pix, G, eps, gm, bt, silu=True, x1=a1, two_pass=False, n_split=ns // 2 * 2)
            if kind == "channel":
                ss = ops.gn_finalize(ops.gn_partial(a0, C, n, pix, ns, x1=a1), G, eps, gm, bt)
                return ops.gn_apply(a0, ss, pix, True, x1=a1)
            return ops.group_norm(a0, n, pix, G, eps, gm, bt, silu=True, x1=a1, two_pass=False, rev3=rev3)
        out = mk.out((n * pix, C), unaligned=False)
        ss = mk.ws(n * C * 8, "scale/shift")
        xa = (a0.data_ptr(), a0.stride(0), c0, a1.data_ptr(), a1.stride(0), C)
        if kind == "group":
            ws = mk.ws(n * ns * G * 16, "group records")
            check(L.vd_gn_partial_g(*xa, n, pix, ns, G, ws.data_ptr(), st()), "vd_gn_partial_g")
            check(L.vd_gn_finalize_g(ws.data_ptr(), n, ns, C, G, eps, gm.data_ptr(), bt.data_ptr(), ss.data_ptr(), st()),
                  "vd_gn_finalize_g")
            check(L.vd_gn_apply_rev3(*xa, n, pix, ss.data_ptr(), 1, out.data_ptr(), out.stride(0), *rev3, st()),
                  "vd_gn_apply_rev3")
        elif kind == "channel":
            ws = mk.ws(n * ns * C * 16, "channel records")
            check(L.vd_gn_partial(*xa, n, pix, ns, ws.data_ptr(), st()), "vd_gn_partial")
            check(L.vd_gn_finalize(ws.data_ptr(), n, ns, C, G, eps, gm.data_ptr(), bt.data_ptr(), ss.data_ptr(), st()),
                  "vd_gn_finalize")
            check(L.vd_gn_apply(*xa, n, pix, ss.data_ptr(), 1, out.data_ptr(), out.stride(0), st()), "vd_gn_apply")
        else:  # two "ranks", each with half of every instance's pixels, records rank-major
            nsl, half = ns // 2, pix // 2
            ws = mk.ws(2 * n * nsl * G * 16, "rank-major records")
            for r in range(2):
                h0 = mk.rows(x0.view(n, 2, half, c0)[:, r].reshape(-1, c0), f"x0 of rank {r}")
                h1 = mk.rows(x1.view(n, 2, half, C - c0)[:, r].reshape(-1, C - c0), f"x1 of rank {r}")
                check(L.vd_gn_partial_g(h0.data_ptr(), h0.stride(0), c0, h1.data_ptr(), h1.stride(0), C, n, half, nsl, G,
                                        ws.data_ptr() + r * n * nsl * G * 16, st()), "vd_gn_partial_g")
            check(L.vd_gn_finalize_g_ranks(ws.data_ptr(), n, 2, nsl, C, G, eps, gm.data_ptr(), bt.data_ptr(),
                                           ss.data_ptr(), st()), "vd_gn_finalize_g_ranks")
            check(L.vd_gn_apply_rev3(*xa, n, pix, ss.data_ptr(), 1, out.data_ptr(), out.stride(0), 1, 1, 0, st()),
                  "vd_gn_apply_rev3")
        return out

    # the rank-major records cover each instance's pixels in another order of splits than the
    # plain call's: equal statistics to fp32 rounding, not bit for bit
    (got,) = run(fn, slack, bitwise=kind != "ranks")
    want = gn_ref(torch.cat([x0, x1], 1), n, pix, C, G, gam, bet, eps, True)
    close_bf16(got, rev3_reference(want, *rev3) if rev3 else want)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("C", [128, 320, 1152, 2048])
def test_res_ln_mod(cuda, slack, C):
    """vd_res_ln_mod: gate / shift / scale as fp32 row views inside one framed modulation buffer
    (ld_mod % 4: the odd slack applies to it), x_out = x in place, rows 70, rows_per_b 35."""
    rows, B = 70, 2
    g = gen(C)
    x, y = rnd(rows, C, g=g), rnd(rows, C, g=g)
    mod = torch.randn(B, 3 * C, device=cuda, generator=g) * 0.5

    def fn(mk):
        xc, m = mk.rows(x, "x"), mk.rows(mod, "mod", unaligned=True)
        h = mk.out((rows, C), unaligned=False)
        ops.res_ln_mod(xc, y=mk.rows(y, "y"), gate=m[:, :C], shift=m[:, C:2 * C], scale=m[:, 2 * C:], rows_per_b=35,
                       x_out=xc, out=h)
        return h, xc

    h, xo = run(fn, slack)
    b = torch.arange(rows, device=cuda) // 35
    xn = x.float() + mod[:, :C][b] * y.float()
    torch.testing.assert_close(xo.float(), xn, rtol=2 ** -7, atol=1e-2)
    want = F.layer_norm(xo.float(), (C,), eps=1e-6) * (1 + mod[:, 2 * C:][b]) + mod[:, C:2 * C][b]
    torch.testing.assert_close(h.float(), want, rtol=2 ** -7, atol=2e-2)


# ---------------------------------------------------------------- attention
def sdpa_ref(q, k, v, batch, heads, sq, skv, d, kv_div=1, scale=None):
    q = q.double().reshape(batch, sq, heads, d).transpose(1, 2)
    kb = k.double().reshape(batch // kv_div, skv, heads, d).transpose(1, 2).repeat_interleave(kv_div, 0)
    vb = v.double().reshape(batch // kv_div, skv, heads, d).transpose(1, 2).repeat_interleave(kv_div, 0)
    w = torch.softmax(q @ kb.transpose(-1, -2) * (d ** -0.5 if scale is None else scale), -1)
    return (w @ vb).transpose(1, 2).reshape(batch * sq, heads * d)


def exp2_ref(q, k, v, batch, heads, sq, skv, d, kv_div):
    """fp64 softmax in log2 units at unit scale (the fp32-output tests' reference)."""
    qd = q.double().reshape(batch, sq, heads, d).transpose(1, 2)
    kd = k.double().reshape(batch // kv_div, skv, heads, d).transpose(1, 2).repeat_interleave(kv_div, 0)
    vd = v.double().reshape(batch // kv_div, skv, heads, d).transpose(1, 2).repeat_interleave(kv_div, 0)
    s = qd @ kd.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return ((p @ vd) / p.sum(-1, keepdim=True)).transpose(1, 2).reshape(batch * sq, heads * d)


def flash512_ref(q, k, v, batch, sq, skv, kv_div):
    """tests/test_gpu_vae.py's fp64 restatement of flash512_kernel (offset m = the first 32-key
    tile's row max, P = bf16(2^(s - m)) for P.V, the row sum over the unrounded values) and its
    rounding-flip allowance, for a K / V shared by kv_div query batches."""
    outs, slacks = [], []
    for i in range(batch):
        qi = q[i * sq:(i + 1) * sq].double()
        j = i // kv_div
        ki, vi = k[j * skv:(j + 1) * skv].double(), v[j * skv:(j + 1) * skv].double()
        s = qi @ ki.T
        e = torch.exp2(s - s[:, :32].amax(1, keepdim=True))
        p = e.float().to(BF).double()
        l = e.sum(1, keepdim=True)
        _, ex = torch.frexp(e)
        ulp = torch.ldexp(torch.full_like(e, 2.0 ** -8), ex)
        mid = (torch.floor(e / ulp) + 0.5) * ulp
        dp = torch.where((e - mid).abs() <= e * 2.0 ** -15, ulp, torch.zeros_like(e))
        outs.append((p @ vi) / l)
        slacks.append((dp @ vi.abs()) / l)
    return torch.cat(outs), torch.cat(slacks)


ATTN_SHAPES = [(200, 333), (300, 77), (64, 1), (130, 130)]


# the family a forced kernel names at a head width that has more than one kernel
ATTN_FORCED = {("v1", 40): "flash", ("flash32", 40): "flash32", ("flash40", 40): "flash40", ("flash40", 80): "flash80"}


def attn_kernels(d, sq, skv):
    """The kernels to ask for: at d = 40 / 80 every forced kernel whose family the plan
    (ops.attention_plan: host only) says runs this shape on a dense, aligned output — elsewhere the
    request falls through to another kernel of the list; "auto" where there is one kernel."""
    names = {40: ["v1", "flash32", "flash40"], 80: ["auto", "flash40"]}.get(d, ["auto"])
    def runs(n):
        return ops.attention_plan(None, None, None, 2, 2, sq, skv, d, kernel=n).family == ATTN_FORCED[n, d]

    return [n for n in names if n == "auto" or runs(n)]


ATTN_CASES = [(d, sq, skv, kern) for d in (32, 40, 64, 80, 128, 160, 512) for sq, skv in ATTN_SHAPES
              for kern in attn_kernels(d, sq, skv)]


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("d,sq,skv,kern", ATTN_CASES)
def test_attention(cuda, slack, out_f32, d, sq, skv, kern):
    """ops.attention: sq == skv is self-attention on column slices of ONE framed fused-QKV buffer
    (batch 2: the query / key tail of instance 0 abuts instance 1's rows, that of instance 1 the
    frame), the others cross-attention with a K / V shared by kv_div = 2 query batches (batch 4).
    bf16 output on N(0, 1.5^2) data against fp64 SDPA; fp32 output on integer scores at the unit
    scale against fp64 at rtol 1e-3 / atol 1e-4 (d = 512: its own restatement and bounds).  `out`
    is a slack-column view (the odd slack: ldo % 8 == 4, except for d = 512's bf16 output, whose
    launcher refuses an ldo that is no multiple of 8: it keeps 8).  A forced kernel runs its own
    family (the plan says so) unless `out`'s rows are not 16-byte ones, which only the 16x16x32
    kernel stores: that fall-through is framed like any other call."""
    heads = 1 if d == 512 else 2
    C = heads * d
    self_attn = sq == skv
    batch, kv_div = (2, 1) if self_attn else (4, 2)
    g = gen(d + sq + skv)
    if d == 512:
        qkv = torch.randn(batch * sq, 3 * C, device=cuda, generator=g)
        qkv[:, :C] *= 0.06
        qf, kvf, scale = qkv[:, :C].to(BF), torch.randn(batch // kv_div * skv, 2 * C, device=cuda, generator=g).to(BF), 1 / LOG2E
        if self_attn:
            kvf = qkv[:, C:].to(BF)
    elif out_f32:
        qf = torch.randint(-1, 2, (batch * sq, C), device=cuda, generator=g).to(BF)
        kvf = torch.cat([torch.randint(-1, 2, (batch // kv_div * skv, C), device=cuda, generator=g).to(BF),
                         rnd(batch // kv_div * skv, C, g=g)], 1)
        scale = 1 / LOG2E
    else:
        qf, kvf, scale = rnd(batch * sq, C, std=1.5, g=g), rnd(batch // kv_div * skv, 2 * C, std=1.5, g=g), None

    def fn(mk):
        if self_attn:
            buf = mk.rows(torch.cat([qf, kvf], 1), "qkv")
            q, k, v = buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:]
        else:
            q, kv = mk.rows(qf, "q"), mk.rows(kvf, "kv")
            k, v = kv[:, :C], kv[:, C:]
        out = mk.out((batch * sq, C), F32 if out_f32 else BF, unaligned=out_f32 or d != 512)
        kw = dict(kv_div=kv_div, scale=scale, out=out, out_f32=out_f32, kernel=kern)
        if kern != "auto":
            rows16 = out.data_ptr() % 16 == 0 and out.stride(0) * out.element_size() % 16 == 0
            assert ops.attention_plan(q, k, v, batch, heads, sq, skv, d, **kw).family == \
                (ATTN_FORCED[kern, d] if rows16 else "flash")
        ops.attention(q, k, v, batch, heads, sq, skv, d, **kw)
        return out

    (got,) = run(fn, slack)
    k, v = kvf[:, :C], kvf[:, C:]
    if d == 512:
        want, allow = flash512_ref(qf, k, v, batch, sq, skv, kv_div)
        err = (got.double() - want).abs()
        assert torch.all(err <= 1e-4 + (1e-3 if out_f32 else 2 ** -8) * want.abs() + allow), err.max().item()
    elif out_f32:
        want = exp2_ref(qf, k, v, batch, heads, sq, skv, d, kv_div)
        err = (got.double() - want).abs()
        assert torch.all(err <= 1e-4 + 1e-3 * want.abs()), err.max().item()
    else:
        close_bf16(got, sdpa_ref(qf, k, v, batch, heads, sq, skv, d, kv_div=kv_div))


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("out_f32", [False, True])
def test_attention_flash40_fixup(cuda, slack, out_f32):
    """flash40's NaN flags and flash32's exact fix-up launch inside poisoned frames, on spike shape
    A of tests/test_gpu_kernels.py (batch 2, heads 3, sq 300, skv 640; four of the six heads
    overflow the fast pass in every 256-query quarter): a flag per 128 queries must land inside
    `out`, the fix-up's second workgroup holds 2 of 16 blocks, and its last block has 44 rows.
    Frames intact, `out` written everywhere (a flagged block the fix-up skipped keeps its poison),
    the result within the deferred-max bar of fp64 SDPA.  As in test_attention, an `out` whose
    rows are not 16-byte ones (the odd slack, bf16) goes to the 16x16x32 kernel instead."""
    from test_gpu_kernels import _spike_shape

    (batch, heads, sq, skv, kv_div), _, (qf, kf, vf) = _spike_shape("A")
    d, C = 40, heads * 40

    def fn(mk):
        q, k, v = mk.rows(qf, "q"), mk.rows(kf, "k"), mk.rows(vf, "v")
        out = mk.out((batch * sq, C), F32 if out_f32 else BF)
        kw = dict(kv_div=kv_div, out=out, out_f32=out_f32, kernel="flash40")
        rows16 = out.data_ptr() % 16 == 0 and out.stride(0) * out.element_size() % 16 == 0
        assert ops.attention_plan(q, k, v, batch, heads, sq, skv, d, **kw).family == ("flash40" if rows16 else "flash")
        ops.attention(q, k, v, batch, heads, sq, skv, d, **kw)
        return out

    (got,) = run(fn, slack)
    want = sdpa_ref(qf, kf, vf, batch, heads, sq, skv, d, kv_div=kv_div)
    close_bf16(got, want, abs_frac=2e-3 * vf.float().abs().max().item() / want.abs().max().item())


@pytest.mark.parametrize("out_f32", [False, True])
def test_attention_abi_entry_points(cuda, out_f32):
    """vd_attention / vd_attention_f32 (the entry points without the kernel choice) through lib():
    d = 64, sq 130, skv 77, batch 2."""
    batch, heads, sq, skv, d = 2, 2, 130, 77, 64
    C = heads * d
    g = gen(9)
    qf = torch.randint(-1, 2, (batch * sq, C), device=cuda, generator=g).to(BF)
    kvf = torch.cat([torch.randint(-1, 2, (batch * skv, C), device=cuda, generator=g).to(BF), rnd(batch * skv, C, g=g)], 1)

    def fn(mk):
        q, kv = mk.rows(qf, "q"), mk.rows(kvf, "kv")
        out = mk.out((batch * sq, C), F32 if out_f32 else BF)
        entry = lib().vd_attention_f32 if out_f32 else lib().vd_attention
        check(entry(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), kv[:, C:].data_ptr(), kv.stride(0),
                    out.data_ptr(), out.stride(0), batch, heads, sq, skv, d, 1, 1 / LOG2E,
                    torch.cuda.current_stream().cuda_stream), "vd_attention")
        return out

    for slack in SLACKS:
        (got,) = run(fn, slack)
        want = exp2_ref(qf, kvf[:, :C], kvf[:, C:], batch, heads, sq, skv, d, 1)
        if out_f32:
            assert torch.all((got.double() - want).abs() <= 1e-4 + 1e-3 * want.abs())
        else:
            close_bf16(got, want)


# ---------------------------------------------------------------- temporal / motion attention
def temporal_ref(q, k, v, batch, qf, kf, pos, heads, d, scale=None):
    C = heads * d

    def tok(t, f):  # rows (b, f, p) -> (b*p, f, C)
        return t.double().reshape(batch, f, pos, C).permute(0, 2, 1, 3).reshape(batch * pos, f, C)

    want = sdpa_ref(tok(q, qf), tok(k, kf), tok(v, kf), batch * pos, heads, qf, kf, d, scale=scale)
    return want.reshape(batch, pos, qf, C).permute(0, 2, 1, 3).reshape(-1, C)


@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("valu", [False, True])
@pytest.mark.parametrize("frames", [5, 16])
@pytest.mark.parametrize("d", [40, 160])
def test_temporal_attention(cuda, slack, valu, frames, d):
    """vd_temporal_attention / _valu on column slices of a framed fused-QKV buffer: batch 2, 37
    positions (items = 2 x 37 x 3 heads: the last workgroup's idle waves), 5 frames (the MFMA
    tile's rows past the frame count)."""
    batch, pos, heads = 2, 37, 3
    C = heads * d
    qkv = rnd(batch * frames * pos, 3 * C, std=1.5, g=gen(frames + d))

    def fn(mk):
        b = mk.rows(qkv, "qkv")
        out = mk.out((batch * frames * pos, C), unaligned=False)
        ops.temporal_attention(b[:, :C], b[:, C:2 * C], b[:, 2 * C:], batch, frames, pos, heads, d, out=out, valu=valu)
        return out

    (got,) = run(fn, slack)
    close_bf16(got, temporal_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], batch, frames, frames, pos, heads, d))


@pytest.mark.parametrize("slack", SLACKS)
def test_temporal_attention_rope(cuda, slack):
    """vd_temporal_attention_rope: 24 frames (8 short of the 32-frame tile), d = 64; q / k rows
    stay un-rotated; against fp32 SDPA of the oracle-rotated operands at the bound of
    tests/test_gpu_dit.py."""
    from oracle import dit_ref
    B, Fr, P, heads, d = 2, 24, 12, 3, 64
    D = heads * d
    qkv = torch.randn(B * Fr * P, 3 * D, generator=torch.Generator().manual_seed(64)).to(BF)
    qc = qkv.cuda()

    def fn(mk):
        b = mk.rows(qc, "qkv")
        out = mk.out((B * Fr * P, D))
        ops.temporal_attention(b[:, :D], b[:, D:2 * D], b[:, 2 * D:], B, Fr, P, heads, d, rope_theta=10000.0, out=out)
        return out, b

    got, buf = run(fn, slack)
    assert torch.equal(buf, qc)
    rows = B * Fr * P
    z = qkv.float()[:, :2 * D].reshape(rows, 2 * heads, d)
    zr = dit_ref.rope(z.transpose(0, 1), (torch.arange(rows) // P) % Fr, 10000.0).transpose(0, 1)
    t = torch.cat([zr.reshape(rows, 2 * D), qkv.float()[:, 2 * D:]], 1)
    t = t.reshape(B, Fr, P, 3, heads, d).permute(3, 0, 2, 4, 1, 5)
    want = F.scaled_dot_product_attention(t[0], t[1], t[2]).permute(0, 3, 1, 2, 4).reshape(rows, D)
    torch.testing.assert_close(got.float().cpu(), want, rtol=2 ** -6, atol=1e-2)


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("d", [40, 160])
def test_temporal_attention_kv(cuda, slack, d):
    """vd_temporal_attention_kv: one query frame (f0 = 15) of 16 against all frames' K / V."""
    batch, pos, heads, frames, f0 = 2, 37, 2, 16, 15
    C = heads * d
    g = gen(d)
    qkv = rnd(batch * frames * pos, 3 * C, std=1.5, g=g)
    q1 = qkv[:, :C].reshape(batch, frames, pos, C)[:, f0:f0 + 1].reshape(-1, C)
    kvf = qkv[:, C:]

    def fn(mk):
        kv = mk.rows(kvf, "kv")
        out = mk.out((batch * pos, C))
        ops.temporal_attention_kv(mk.rows(q1, "q"), kv[:, :C], kv[:, C:], batch, 1, frames, pos, heads, d, out=out)
        return out

    (got,) = run(fn, slack)
    close_bf16(got, temporal_ref(q1, kvf[:, :C], kvf[:, C:], batch, 1, frames, pos, heads, d))


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("folded", [False, True])
def test_motion_qkv_attention(cuda, slack, folded):
    """vd_motion_qkv_attention at the smallest ragged position count it takes at batch 2 (the
    last workgroup's idle waves), plain and with the LayerNorm + PE fold; bounds as in
    tests/test_gpu_kernels.py."""
    from vdiff.models.layers import MotionLnFold
    Cc, d, heads, NF, batch = 320, 40, 8, 16, 2
    pos = next(p for p in range(1, 1 << 15) if p % 4 and ops.motion_qkv_takes(batch, NF, p, heads, d))
    assert not ops.motion_qkv_takes(batch, NF, pos - 1, heads, d) or (pos - 1) % 4 == 0
    g = gen(3)
    rows = batch * NF * pos
    x = (1.3 * torch.randn(rows, Cc, device=cuda, generator=g)).to(BF)
    w = torch.randn(3 * Cc, Cc, device=cuda, generator=g) * Cc ** -0.5 * 2.0
    sc = 1.0 / LOG2E
    if folded:
        norm = torch.nn.LayerNorm(Cc).to(cuda)
        with torch.no_grad():
            norm.weight.copy_(1 + 0.2 * torch.randn(Cc, device=cuda, generator=g))
            norm.bias.copy_(0.1 * torch.randn(Cc, device=cuda, generator=g))
        pe = torch.randn(32, Cc, device=cuda, generator=g) * 0.5
        fold = MotionLnFold(norm, w, pe, heads, d)
        wk = fold.w
    else:
        wk = w.to(BF)

    def fn(mk):
        out = mk.out((rows, Cc))
        got = ops.motion_qkv_attention(mk.rows(x, "x"), mk.rows(wk, "wqkv"), batch, NF, pos, heads, d, scale=sc, out=out,
                                       ln_fold=(mk.flat(fold.tab, "fold table"), fold.eps) if folded else None)
        assert got is not None
        return out

    (got,) = run(fn, slack)
    if folded:
        ln = F.layer_norm(x.double(), (Cc,), norm.weight.double(), norm.bias.double(), norm.eps)
        qkv = (ln + pe.double()[(torch.arange(rows, device=cuda) // pos) % NF]) @ w.double().T
    else:
        qkv = ops.gemm(x, wk).double()  # the bf16 projection the fused kernel reproduces bit for bit
    q, k, v = qkv[:, :Cc] * (sc * math.sqrt(d)), qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
    ref = temporal_ref(q, k, v, batch, NF, NF, pos, heads, d)
    if folded:
        assert ((got.double() - ref).norm() / ref.norm()).item() < 2.5e-2
    else:
        close_bf16(got, ref)


# ---------------------------------------------------------------- fp8 attention, softmax
@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("rope", [False, True])
def test_attention_fp8(cuda, slack, rope):
    """ops.attention_fp8 (quantisation + attention), its fp8 buffers and scales from the wrapper's
    poisoned torch.empty.  vd_attention_fp8 takes sq % 32 == 0 and skv % 64 == 0 only: sq = skv =
    320 for the listed 300 (16 x 20 RoPE grid), heads 2, batch 2.  Within 10 % rel-L2 of exact fp32
    SDPA (the bound of tests/test_gpu_dit.py), finite everywhere."""
    from oracle import dit_ref
    B, heads, Hp, Wp, d = 2, 2, 16, 20, 64
    S, D = Hp * Wp, heads * d
    qkv = (torch.randn(B * S, 3 * D, generator=torch.Generator().manual_seed(11)) * 1.5).to(BF)
    qc = qkv.cuda()

    def fn(mk):
        b = mk.rows(qc, "qkv")
        out = mk.out((B * S, D))
        ops.attention_fp8(b[:, :D], b[:, D:2 * D], b[:, 2 * D:], B, heads, S, S, d, out=out,
                          rope=(Hp, Wp, 10000.0) if rope else None)
        return out, b

    got, buf = run(fn, slack)
    assert torch.equal(buf, qc)
    x = qkv.float()
    if rope:
        r = torch.arange(B * S)
        z = x[:, :2 * D].reshape(B * S, 2 * heads, d)
        zh = dit_ref.rope(z[..., :d // 2].transpose(0, 1), (r // Wp) % Hp, 10000.0).transpose(0, 1)
        zw = dit_ref.rope(z[..., d // 2:].transpose(0, 1), r % Wp, 10000.0).transpose(0, 1)
        x = torch.cat([torch.cat([zh, zw], -1).reshape(B * S, 2 * D), x[:, 2 * D:]], 1)
    t = x.reshape(B, S, 3, heads, d).permute(2, 0, 3, 1, 4)
    want = F.scaled_dot_product_attention(t[0], t[1], t[2]).permute(0, 2, 1, 3).reshape(B * S, D)
    g = got.float().cpu()
    assert torch.isfinite(g).all()
    assert ((g - want).norm() / want.norm()).item() < 0.10


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("cols", [76, 4100])
def test_softmax_rows(cuda, slack, cols):
    """vd_softmax_rows on strided s and out.  cols % 4 == 0 is required: 76 for the listed 77
    (one partial pass of the 1024-column step), 4100 (five passes, the last of one float4)."""
    rows = 5
    s = torch.randn(rows, cols, device=cuda, generator=gen(cols)) * 6

    def fn(mk):
        out = mk.out((rows, cols))
        return ops.softmax_rows(mk.rows(s, "s", unaligned=True), out=out)

    (got,) = run(fn, slack)
    torch.testing.assert_close(got.double(), torch.softmax(s.double() * math.log(2.0), -1), rtol=2 ** -7, atol=1e-6)


# ---------------------------------------------------------------- row ops
@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("y_f32", [False, True])
def test_rows_add(cuda, slack, with_x, y_f32):
    """vd_rows_eltwise(add): x None / given, y bf16 / fp32 with y_div and y_period, out a column
    slice; 77 rows of 72 channels.  Only an fp32 y may have a row stride that is no multiple of 8."""
    rows, Cc, y_div, period = 77, 72, 5, 4
    g = gen(1)
    x = rnd(rows, Cc, g=g)
    y = torch.randn(6, Cc, device=cuda, generator=g)
    y = y if y_f32 else y.to(BF)

    def fn(mk):
        out = mk.out((rows, Cc), unaligned=False)
        return ops.rows_add(mk.rows(x, "x") if with_x else None, mk.rows(y, "y", unaligned=y_f32), y_div=y_div,
                            y_period=period, out=out)

    (got,) = run(fn, slack)
    want = y.double()[(torch.arange(rows, device=cuda) // y_div) % period] + (x.double() if with_x else 0)
    close_bf16(got, want)


@pytest.mark.parametrize("slack", (0, 8))
def test_silu_rows(cuda, slack):
    x = rnd(77, 72, std=2.0, g=gen(2))

    def fn(mk):
        return ops.silu_rows(mk.rows(x, "x"), out=mk.out((77, 72), unaligned=False))

    (got,) = run(fn, slack)
    close_bf16(got, F.silu(x.double()))


@pytest.mark.parametrize("slack", (0, 8))
def test_upsample2x_rows(cuda, slack):
    n, h, w, Cc = 2, 5, 3, 72
    x = rnd(n * h * w, Cc, g=gen(3))

    def fn(mk):
        return ops.upsample2x_rows(mk.rows(x, "x"), n, h, w, out=mk.out((n * 4 * h * w, Cc), unaligned=False))

    (got,) = run(fn, slack)
    want = x.reshape(n, h, 1, w, 1, Cc).expand(n, h, 2, w, 2, Cc).reshape(-1, Cc)
    assert torch.equal(got, want)


def test_block_transpose(cuda):
    from vdiff.dist import block_transpose_reference
    src = rnd(2 * 3 * 5, 16, g=gen(4))

    def fn(mk):
        out = mk.out((30, 16), slack=0)
        return ops.block_transpose(mk.rows(src, "src", slack=0), 2, 3, 5, out=out)

    (got,) = run(fn, 0)
    assert torch.equal(got, block_transpose_reference(src, 2, 3, 5))


# ---------------------------------------------------------------- step glue
def test_pack_unpack(cuda):
    """vd_pack_latents (dup 2, cpad 8) and vd_unpack_nhwc from a bf16 and an fp32 source with a
    row stride."""
    g = gen(5)
    x = torch.randn(2, 4, 3, 8, 6, device=cuda, generator=g)
    n = 2 * 3 * 48

    def pack(mk):
        return ops.pack_latents(mk.flat(x, "latents"), dup=2, cpad=8, out=mk.out((2 * n, 8), slack=0))

    (rows,) = run(pack, 0)
    assert torch.all(rows[:, 4:] == 0) and torch.equal(rows[:n], rows[n:])
    want = x.permute(0, 2, 3, 4, 1).reshape(n, 4)
    close_bf16(rows[:n, :4], want)
    for slack in (0, 8, 2):
        for src in (rows[:n], torch.randn(n, 4, device=cuda, generator=g)):
            def unpack(mk, src=src):
                return ops.unpack_nhwc(mk.rows(src, "src", unaligned=True), 2, 4, 3, 8, 6,
                                       out=mk.out_flat((2, 4, 3, 8, 6), F32))
            (back,) = run(unpack, slack)
            assert torch.equal(back, src[:, :4].float().reshape(2, 3, 8, 6, 4).permute(0, 4, 1, 2, 3))


def test_timestep_embed(cuda):
    from oracle.unet_ref import timestep_embedding
    ts = torch.tensor([961.0, 1.0, 500.0], device=cuda)
    step = torch.tensor([2], device=cuda, dtype=torch.int32)

    def plain(mk):
        return ops.timestep_embed(mk.flat(ts, "ts"), 320, out=mk.out((3, 320)))

    def indexed(mk):
        return ops.timestep_embed(mk.flat(ts, "ts"), 320, step_idx=mk.flat(step, "step"), batch=2, out=mk.out((2, 320)))

    for slack in (0,):  # the output is addressed as contiguous rows of `dim`
        close_bf16(run(plain, slack)[0], timestep_embedding(ts.cpu(), 320))
        close_bf16(run(indexed, slack)[0], timestep_embedding(torch.tensor([500.0, 500.0]), 320))


@pytest.mark.parametrize("sched", ["ddim", "euler"])
def test_cfg_step(cuda, sched):
    """vd_ddim_cfg_step / vd_euler_cfg_step: latents updated in place inside a frame, x0_out and
    next_in framed, eps rows with a row stride; against the oracles at their tests' bounds."""
    from oracle import ddim_ref, euler_ref
    B, Cc, Fr, H, W = 1, 4, 3, 8, 8
    g = gen(6)
    n = Fr * H * W
    eps_rows = torch.randn(2 * n, 4, device=cuda, generator=g)
    if sched == "ddim":
        acp = ddim_ref.alphas_cumprod()
        t, steps = 961, 50
        prev = t - 1000 // steps
        sq = ddim_ref._sqrt
        coef = torch.stack([sq(acp[t]), sq(1 - acp[t]), sq(acp[prev]), sq(1 - acp[prev])]).float()
        lat = torch.randn(B, Cc, Fr, H, W, device=cuda, generator=g)
    else:
        _, sig = euler_ref.set_timesteps(25)
        s, sn = sig[11], sig[12]
        coef = torch.stack([s, sn, (sn ** 2 + 1) ** 0.5, torch.zeros(())]).float()
        lat = torch.randn(B, Cc, Fr, H, W, device=cuda, generator=g) * float(s)

    def fn(mk):
        x = mk.flat(lat, "latents")
        x0 = mk.out_flat((B, Cc, Fr, H, W), F32, "x0_out")
        nxt = mk.out((2 * n, 8), name="next_in", slack=0)
        ops.SCHED_STEP[sched](mk.rows(eps_rows, "eps", unaligned=True), 2, 7.5, x, mk.flat(coef.to(cuda), "coef"),
                              x0_out=x0, next_in=nxt)
        return x, x0, nxt

    for slack in (0, 2):
        x, x0, nxt = run(fn, slack)
        e = eps_rows.cpu().reshape(2, Fr, H, W, 4).permute(0, 4, 1, 2, 3)
        if sched == "ddim":
            want, want0 = ddim_ref.ddim_step(ddim_ref.cfg_combine(e, 7.5), t, lat.cpu(), steps, acp)
            assert torch.equal(x.cpu(), want) and torch.equal(x0.cpu(), want0)
            nref = want
        else:
            e = e[0:1] + 7.5 * (e[1:2] - e[0:1])
            want, want0 = euler_ref.euler_step(e, lat.cpu(), s, sn)
            close_f32(x, want, rtol=1e-6, atol=1e-6)
            close_f32(x0, want0, rtol=1e-6, atol=1e-6)
            nref = euler_ref.scale_model_input(want, sn)
        assert torch.equal(nxt[:n], nxt[n:]) and torch.all(nxt[:, 4:] == 0)
        close_bf16(nxt[:n, :4], nref.permute(0, 2, 3, 4, 1).reshape(n, 4))


def test_step_advance(cuda):
    def fn(mk):
        s = mk.flat(torch.zeros(1, device=cuda, dtype=torch.int32), "step_idx")
        ops.step_advance(s)
        ops.step_advance(s)
        return s

    (s,) = run(fn, 0)
    assert s.item() == 2


@pytest.mark.parametrize("shape,p,dup", [((2, 4, 3, 12, 20), 2, 2), ((1, 3, 2, 9, 6), 3, 1)])
def test_patchify_unpatchify(cuda, shape, p, dup):
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(shape, generator=g)
    B, Cc, Fr, H, W = shape
    kpad = (Cc * p * p + 7) // 8 * 8
    n = B * Fr * (H // p) * (W // p)

    def pat(mk):
        return ops.patchify(mk.flat(lat.cuda(), "latents"), p, kpad, dup=dup, in_div=2.0, out=mk.out((dup * n, kpad), slack=0))

    tok = run(pat, 0)[0].float().cpu()
    ref = lat.reshape(B, Cc, Fr, H // p, p, W // p, p).permute(0, 2, 3, 5, 1, 4, 6)
    ref = (ref.reshape(-1, Cc * p * p) / 2.0).to(BF).float()
    assert torch.equal(tok[:n, :Cc * p * p], ref) and not tok[:, Cc * p * p:].any()
    assert dup == 1 or torch.equal(tok[n:], tok[:n])
    src = torch.randn(n, p * p * Cc, generator=g)

    def unpat(mk):
        return ops.unpatchify(mk.rows(src.cuda(), "src", unaligned=True), B * Fr, H, W, p, Cc,
                              out=mk.out((B * Fr * H * W, Cc), F32, slack=0))

    for slack in (0, 8, 2):
        pix = run(unpat, slack)[0].cpu()
        want = src.reshape(B * Fr, H // p, W // p, p, p, Cc).permute(0, 1, 3, 2, 4, 5)
        assert torch.equal(pix, want.reshape(-1, Cc))


@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("mode", [0, 1])
def test_rope_qk(cuda, slack, mode):
    """vd_rope_qk in place on the q | k column subset of framed fused-QKV rows: v untouched."""
    from oracle import dit_ref
    B, Fr, Hp, Wp, heads, d = 2, 5, 6, 7, 3, 64
    D, rows = heads * d, 2 * 5 * 6 * 7
    qkv = torch.randn(rows, 3 * D, generator=torch.Generator().manual_seed(1)).to(BF)

    def fn(mk):
        return ops.rope_qk(mk.rows(qkv.cuda(), "qkv"), 2 * D, d, mode, Fr, Hp, Wp, 10000.0)

    got = run(fn, slack)[0].float().cpu()
    r = torch.arange(rows)
    z = qkv.float()[:, :2 * D].reshape(rows, 2 * heads, d)
    if mode == 0:
        zh = dit_ref.rope(z[..., :d // 2].transpose(0, 1), (r // Wp) % Hp, 10000.0).transpose(0, 1)
        zw = dit_ref.rope(z[..., d // 2:].transpose(0, 1), r % Wp, 10000.0).transpose(0, 1)
        want = torch.cat([zh, zw], -1)
    else:
        want = dit_ref.rope(z.transpose(0, 1), (r // (Hp * Wp)) % Fr, 10000.0).transpose(0, 1)
    torch.testing.assert_close(got[:, :2 * D].reshape(rows, 2 * heads, d), want, rtol=2 ** -7, atol=2e-2)
    assert torch.equal(got[:, 2 * D:], qkv.float()[:, 2 * D:])


# ---------------------------------------------------------------- metrics
def smooth_video(g, V, Fr, H, W, shift=1.0):
    """tests/test_gpu_lpips.py's band-limited random texture translated by `shift` px per frame."""
    base = torch.randn(V, 3, H + 8 * Fr, W + 8 * Fr, generator=g)
    base = F.avg_pool2d(F.avg_pool2d(base, 5, 1, 2), 5, 1, 2)
    v = torch.stack([base[:, :, int(round(f * shift)):int(round(f * shift)) + H,
                          int(round(f * shift)):int(round(f * shift)) + W] for f in range(Fr)], 1)
    v = (v - v.amin()) / (v.amax() - v.amin())
    return (v.permute(0, 1, 3, 4, 2) * 255).round().to(torch.uint8).contiguous()


def test_frame_sums(cuda):
    from oracle import metrics_ref
    from vdiff import metrics
    x = torch.randint(0, 256, (2, 3, 24, 40, 3), generator=torch.Generator().manual_seed(203), dtype=torch.uint8)
    x[0, 0], x[0, 1] = 255, 0

    def fn(mk):
        return metrics.frame_sums(mk.flat(x.cuda(), "videos"))

    sse, sad = run(fn, 0)
    for v in range(2):
        assert sse[v].cpu().tolist() == metrics_ref.pair_sse(x[v].numpy()).tolist()
        assert sad[v].cpu().tolist() == metrics_ref.triplet_sad(x[v].numpy()).tolist()


@pytest.mark.parametrize("via", ["wrapper", "abi"])
def test_farneback_flow_and_sums(cuda, via):
    """vd_farneback_flow + vd_flow_warp_stats on (2, 3, 24, 40): through vdiff.metrics under
    poisoned_empty, and through lib() with framed workspaces of exactly the advertised sizes and
    a framed flow; against oracle/flow_ref.py at the bounds of tests/test_gpu_metrics.py."""
    import numpy as np
    from oracle import flow_ref
    from vdiff import metrics
    V, Fr, H, W = 2, 3, 24, 40
    x = smooth_video(torch.Generator().manual_seed(H * W + Fr), V, Fr, H, W)
    x[0, -1, :4] = 255
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def fn(mk):
        xc = mk.flat(x.cuda(), "videos")
        if via == "wrapper" or not mk.framed:
            flow = metrics.farneback_flow(xc)
            return flow, metrics.flow_sums(xc, flow)
        p = metrics.FARNEBACK
        nb = lib().vd_farneback_workspace(V, Fr, H, W)
        ws = mk.ws(nb, "farneback workspace")
        flow = mk.out_flat((V, Fr - 1, H, W, 2), F32, "flow")
        check(lib().vd_farneback_flow(xc.data_ptr(), V, Fr, H, W, p["pyr_scale"], p["levels"], p["winsize"],
                                      p["iterations"], p["poly_n"], p["poly_sigma"], flow.data_ptr(), ws.data_ptr(), nb,
                                      st()), "vd_farneback_flow")
        nb2 = lib().vd_flow_warp_workspace(V, Fr)
        ws2 = mk.ws(nb2, "warp workspace")
        stats = mk.out_flat((V, Fr - 1, 3), torch.float64, "stats")
        check(lib().vd_flow_warp_stats(xc.data_ptr(), flow.data_ptr(), V, Fr, H, W, stats.data_ptr(), ws2.data_ptr(),
                                       nb2, st()), "vd_flow_warp_stats")
        return flow, stats

    flow, stats = run(fn, 0)
    flow, stats = flow.cpu().numpy(), stats.cpu().numpy()
    for v in range(V):
        fr = x[v].permute(0, 3, 1, 2).float() / 255
        for i in range(Fr - 1):
            o = flow_ref.pair_metrics(fr[i], fr[i + 1])
            assert np.abs(flow[v, i] - o["flow"]).max() < 1e-3
            ff = metrics.flow_fields(stats[v, i:i + 1].tolist(), H * W)
            assert ff["mean_flow_magnitude"] == pytest.approx(o["flow_magnitude_mean"], rel=1e-4)
            assert ff["pairs"][0]["flow_magnitude_std"] == pytest.approx(o["flow_magnitude_std"], rel=1e-4)
            assert ff["mean_warp_error"] == pytest.approx(o["warp_error"], rel=1e-4, abs=1e-9)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("cin,cout,k,stride,pad,N,H,W", [(3, 64, 11, 4, 2, 2, 35, 33), (64, 192, 3, 1, 1, 3, 7, 5)])
def test_conv2d_f32(cuda, cin, cout, k, stride, pad, N, H, W, relu):
    """vd_conv2d_f32: AlexNet's first layer form on 35 x 33 and a Cin 64, k 3, pad 1 case with a
    ragged pixel count (105); the bound of tests/test_gpu_lpips.py."""
    import lpips_ref
    g = torch.Generator().manual_seed(cin * 1000 + H * W + k)
    if cin == 3:
        u = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
        u[0, :9, -13:] = 255
        x = lpips_ref.scale_input(u, torch.float32)
    else:
        x = torch.randn(N, cin, H, W, generator=g).clamp_min(0)
        x[0, :, :2, -2:] = x.max()
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride, pad)
    bound = 1e-6 * lpips_ref.conv_bound(x.double(), w.double(), b.double(), stride, pad)
    ref = ref.clamp_min(0) if relu else ref

    def fn(mk):
        out = mk.out_flat((N, ref.shape[2], ref.shape[3], cout), F32)
        return ops.conv2d_f32(mk.flat(x.permute(0, 2, 3, 1).contiguous().cuda(), "x"),
                              mk.flat(w.permute(0, 2, 3, 1).contiguous().cuda(), "w"), mk.flat(b.cuda(), "bias"),
                              stride=stride, pad=pad, relu=relu, out=out)

    (y,) = run(fn, 0)
    err = (y.cpu().double().permute(0, 3, 1, 2) - ref).abs()
    assert bool((err <= bound).all())


@pytest.mark.parametrize("via", ["wrapper", "abi"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_lpips_layer(cuda, via, accumulate):
    """vd_lpips_layer, C 192, 165 pixels, 4 pairs, plain and accumulating onto a framed out; the
    workspace from the wrapper's poisoned torch.empty or framed at exactly the advertised size."""
    import lpips_ref
    Cc, pixels, pairs = 192, 165, 4
    g = torch.Generator().manual_seed(Cc + pixels + pairs)
    fa = torch.randn(pairs, pixels, Cc, generator=g).clamp_min(0)
    fb = torch.randn(pairs, pixels, Cc, generator=g).clamp_min(0)
    fa[:, 1], fa[:, 3], fb[:, 3], fb[:, pixels - 1] = 0, 0, 0, 0
    fb[2] = fa[2]
    lin = torch.randn(Cc, generator=g).abs() / Cc ** 0.5
    base = torch.rand(pairs, generator=g).double()
    ref = lpips_ref.layer_distance(fa.double().permute(0, 2, 1)[..., None], fb.double().permute(0, 2, 1)[..., None],
                                   lin.double())

    def fn(mk):
        a, b, l = mk.flat(fa.cuda(), "fa"), mk.flat(fb.cuda(), "fb"), mk.flat(lin.cuda(), "lin")
        out = mk.flat(base.cuda(), "out") if accumulate else mk.out_flat((pairs,), torch.float64)
        if via == "wrapper" or not mk.framed:
            return ops.lpips_layer(a, b, l, out=out, accumulate=accumulate)
        nb = lib().vd_lpips_layer_workspace(pairs)
        ws = mk.ws(nb, "lpips layer workspace")
        check(lib().vd_lpips_layer(a.data_ptr(), b.data_ptr(), pairs, pixels, Cc, l.data_ptr(), out.data_ptr(),
                                   int(accumulate), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream),
              "vd_lpips_layer")
        return out

    got = run(fn, 0)[0].cpu() - (base if accumulate else 0)
    assert accumulate or got[2].item() == 0.0
    keep = ref > 0
    rel = ((got - ref).abs()[keep] / ref[keep]).max().item()
    assert rel <= 3e-5


@pytest.mark.parametrize("via", ["wrapper", "abi"])
def test_lpips_pairs(cuda, via):
    """LPIPS.synthetic on (2, 2, 35, 33): through the class under poisoned_empty, and through
    lib().vd_lpips_pairs with the feature workspace framed at exactly vd_lpips_workspace bytes;
    the parameter blob framed both times.  Bound: 4x the case's conditioning floor, as
    tests/test_gpu_lpips.py."""
    import lpips_ref
    from vdiff import metrics
    V, Fr, H, W = 2, 2, 35, 33
    alex, lin = lpips_ref.synthetic_state_dicts(1)
    params = metrics.lpips_pack_params(*metrics.lpips_synthetic_state_dicts(1))
    x = torch.randint(0, 256, (V, Fr, H, W, 3), generator=torch.Generator().manual_seed(H * W + Fr), dtype=torch.uint8)

    def fn(mk):
        xc, pc = mk.flat(x.cuda(), "videos"), mk.flat(params.cuda(), "params")
        if via == "wrapper" or not mk.framed:
            return metrics.LPIPS(pc, device=cuda)(xc)
        nb = int(lib().vd_lpips_workspace(V * Fr, H, W))
        ws = mk.ws(nb, "lpips workspace")
        out = mk.out_flat((V, Fr - 1), torch.float64)
        check(lib().vd_lpips_pairs(xc.data_ptr(), V, Fr, H, W, pc.data_ptr(), out.data_ptr(), ws.data_ptr(), nb,
                                   torch.cuda.current_stream().cuda_stream), "vd_lpips_pairs")
        return out

    (got,) = run(fn, 0)
    ref = lpips_ref.lpips_pairs(x, alex, lin)
    floor = lpips_ref.conditioning_floor(x, alex, lin, ref)
    dev = ((got.cpu() - ref).abs() / ref.abs()).max().item()
    assert floor <= 2.5e-5, f"ill-conditioned case (floor {floor:.2e}): the test is misconfigured"
    assert dev <= 4 * floor, f"device deviates {dev:.2e} from fp64, floor {floor:.2e}"
