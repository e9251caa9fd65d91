"""FreeInit on the MI355X: vd_rows_eltwise op 6 (the five-pass 3-D spectral low-pass behind
ops.free_init_filter) against the fp64 reference of tests/free_init_ref.py, its exact and bitwise
properties, framed by tests/memframe.py and under a captured graph; DenoiseLoop.reschedule; and
enable_free_init end to end on the tiny pipelines against the same thing composed by hand.

Kernel bar (set by the reference, never by what the kernel gives): every element within
max(4 * e32, 2^-22 * max|x - noise|) of the fp64 reference, e32 being the max abs error of the
same reference evaluated in fp32 by torch.fft on the CPU for the same inputs.  The device's
closest approach per shape is in DESIGN.md.
"""
import functools
import gc

import pytest
import torch

import free_init_ref as R
import memframe as mf
import vdiff.pipeline as P
from vdiff import (AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline, DDIMScheduler, DenoiseLoop,
                   EulerDiscreteScheduler, ops)

pytestmark = pytest.mark.gpu
F32 = torch.float32
METHODS = ("butterworth", "gaussian", "ideal")

# (n_vol, F, H, W)
SHAPES = [(2, 3, 4, 6),      # odd F
          (8, 4, 8, 8),      # basic even case
          (2, 5, 6, 10),     # odd F, non-power-of-two
          (1, 7, 9, 5),      # all odd, Wh = 3
          (1, 1, 8, 8),      # one frame
          (3, 8, 1, 16),     # H = 1
          (1, 2, 72, 66),    # lines longer than a wavefront and not a multiple of it
          (1, 40, 16, 16),   # FreeNoise-length F, past 32
          (4, 16, 32, 32)]   # mid-size even
PRODUCT = (4, 16, 64, 64)
CASES = [(s, m) for s in SHAPES for m in METHODS] + [(PRODUCT, "butterworth")]
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@functools.lru_cache(maxsize=None)
def inputs(shape, seed=0):
    """fp32 N(0, 1) x and noise from a seeded CPU generator (exact in fp64 as well)."""
    g = torch.Generator().manual_seed(1000 * seed + sum(shape))
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g)


@functools.lru_cache(maxsize=None)
def reference(shape, method):
    """(fp64 reference, e32, max|x - noise|) on the CPU, computed once per case."""
    x, noise = inputs(shape)
    lpf = R._get_free_init_freq_filter((1,) + shape[1:], method, 4, 0.25, 0.25)
    want = R._apply_freq_filter(x.double(), noise.double(), lpf)
    in32 = R._apply_freq_filter(x, noise, lpf.float())
    assert in32.dtype == F32
    return want, (in32.double() - want).abs().max().item(), (x - noise).abs().max().item()


def bar_of(e32, dmax):
    return max(4 * e32, 2.0 ** -22 * dmax)


def table_dev(shape, method="butterworth"):
    return ops.free_init_table(*shape[1:], method, 4, 0.25, 0.25, device="cuda")


def run(shape, method="butterworth", seed=0, **kw):
    x, noise = inputs(shape, seed)
    return ops.free_init_filter(x.cuda(), noise.cuda(), table_dev(shape, method), **kw)


# ---------------------------------------------------------------- error against the fp64 reference
@pytest.mark.parametrize("shape,method", CASES, ids=ids)
def test_filter_matches_fp64_within_four_times_torch_fft_fp32(cuda, shape, method):
    want, e32, dmax = reference(shape, method)
    x, noise = inputs(shape)
    with mf.poisoned_empty():
        got = run(shape, method)
    err = (got.double().cpu() - want).abs()
    bar = bar_of(e32, dmax)
    away_n, away_x = (want - noise.double()).abs().max().item(), (want - x.double()).abs().max().item()
    print(f"free_init {ids(shape)} {method}: max err {err.max().item():.3e}  e32 {e32:.3e}  bar {bar:.3e}  "
          f"ratio to e32 {err.max().item() / e32:.2f}; reference is {away_n:.3g} from noise, {away_x:.3g} from x")
    assert got.shape == x.shape and got.dtype == F32
    bad = int((~(err <= bar)).sum())  # a NaN is outside
    assert bad == 0, f"{bad} of {err.numel()} elements outside {bar:.3e}; max {err.max().item():.3e}"
    # a no-op in either direction is far outside the bar.  (An axis of one point sits at index 0,
    # a full unit from the mask's centre N / 2, so there d^2 >= 1, the mask is ~0 and the reference
    # IS the noise.)
    assert away_x > 100 * bar
    if min(shape[1:]) > 1:
        assert away_n > 100 * bar


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_exact_cases(cuda, shape):
    x, noise = (t.cuda() for t in inputs(shape))
    Fr, H, W = shape[1:]
    zeros = torch.zeros(Fr, H, W // 2 + 1, device="cuda")
    assert torch.equal(ops.free_init_filter(x, noise, zeros), noise)           # n + 0
    assert torch.equal(ops.free_init_filter(noise, noise, table_dev(shape)), noise)  # x = noise
    assert torch.equal(ops.free_init_filter(noise.clone(), noise, table_dev(shape)), noise)
    # a zero stop frequency is the zero table
    assert torch.equal(ops.free_init_filter(x, noise, ops.free_init_table(Fr, H, W, "gaussian", 4, 0, 0.25,
                                                                          device="cuda")), noise)
    # table all ones: the transform pair alone, which returns x
    want, e32, dmax = reference(shape, "butterworth")
    ones = ops.free_init_filter(x, noise, torch.ones_like(zeros))
    err = (ones.double() - x.double()).abs().max().item()
    assert err <= bar_of(e32, dmax), (err, e32)


# ---------------------------------------------------------------- independence, bitwise
@pytest.mark.parametrize("shape", [(8, 4, 8, 8), (2, 5, 6, 10), (3, 8, 1, 16), (4, 16, 32, 32), (2, 3, 72, 66)], ids=ids)
def test_volumes_are_independent_bitwise(cuda, shape):
    x, noise = (t.cuda() for t in inputs(shape))
    tab = table_dev(shape)
    both = ops.free_init_filter(x, noise, tab)
    n = shape[0]
    for i in range(n):  # one by one
        one = ops.free_init_filter(x[i:i + 1].clone(), noise[i:i + 1].clone(), tab)
        assert torch.equal(one[0], both[i]), i
    # another position in the batch, other neighbours
    perm = list(range(n))[::-1]
    rev = ops.free_init_filter(x[perm].contiguous(), noise[perm].contiguous(), tab)
    assert torch.equal(rev, both[perm])
    # leading dims are volumes whatever their grouping
    if n % 2 == 0:
        g = ops.free_init_filter(x.reshape((2, n // 2) + shape[1:]), noise.reshape((2, n // 2) + shape[1:]), tab)
        assert torch.equal(g.reshape(shape), both)


@pytest.mark.parametrize("shape", [(2, 5, 6, 10), (1, 2, 72, 66), (4, 16, 32, 32)], ids=ids)
def test_scratch_and_out_contents_do_not_matter(cuda, shape):
    x, noise = (t.cuda() for t in inputs(shape))
    tab = table_dev(shape)
    want = ops.free_init_filter(x, noise, tab).clone()
    rows, Wh = shape[0] * shape[1] * shape[2], shape[3] // 2 + 1
    scratch = torch.empty(rows * 2 * Wh, device="cuda")
    out = torch.empty_like(x)
    for fill in (float("nan"), 0.0, 1e30):
        scratch.fill_(fill)
        out.fill_(fill)
        assert ops.free_init_filter(x, noise, tab, out=out, scratch=scratch) is out
        assert torch.equal(out, want), fill
    # reused as the last call left them, and with other data in between
    assert torch.equal(ops.free_init_filter(x, noise, tab, out=out, scratch=scratch), want)
    ops.free_init_filter(noise, x, tab, out=out, scratch=scratch)
    assert torch.equal(ops.free_init_filter(x, noise, tab, out=out, scratch=scratch), want)
    with mf.poisoned_empty():
        assert torch.equal(ops.free_init_filter(x, noise, tab), want)


def test_wrapper_refuses_by_name(cuda):
    x, noise = (t.cuda() for t in inputs((2, 3, 4, 6)))
    tab = table_dev((2, 3, 4, 6))
    with pytest.raises(ValueError, match="noise"):
        ops.free_init_filter(x, noise[:1].contiguous(), tab)
    with pytest.raises(ValueError, match="noise"):
        ops.free_init_filter(x, noise.double(), tab)
    with pytest.raises(ValueError, match="free_init_filter z"):
        ops.free_init_filter(x.half(), noise, tab)
    with pytest.raises(ValueError, match="free_init_filter z"):
        ops.free_init_filter(x.transpose(-1, -2), noise.transpose(-1, -2), tab)
    with pytest.raises(ValueError, match="table"):
        ops.free_init_filter(x, noise, tab[:, :, :3].contiguous())
    with pytest.raises(ValueError, match="scratch"):
        ops.free_init_filter(x, noise, tab, scratch=torch.empty(10, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        ops.free_init_filter(x, noise, tab, out=torch.empty(2, 3, 4, 5, device="cuda"))
    odd = torch.zeros(2, 1, 3, 5, device="cuda")  # the second volume starts 60 bytes in
    with pytest.raises(ValueError, match="aligned"):
        ops.free_init_filter(odd[1:], odd[1:].clone(), torch.zeros(1, 3, 3, device="cuda"))
    big = torch.zeros(1, 1, 1, ops.SPECTRAL_MAX + 1, device="cuda")
    with pytest.raises(ValueError, match="limit"):
        ops.free_init_filter(big, big.clone(), torch.zeros(1, 1, ops.SPECTRAL_MAX // 2 + 1, device="cuda"))


# ---------------------------------------------------------------- framed
@pytest.mark.parametrize("shape", [(2, 3, 4, 6), (1, 2, 72, 66)], ids=ids)
def test_filter_framed(cuda, shape):
    x, noise = inputs(shape)
    want, e32, dmax = reference(shape, "butterworth")
    rows, Wh = shape[0] * shape[1] * shape[2], shape[3] // 2 + 1
    xv, xf = mf.loadnd(x.cuda(), name="x")
    nv, nf = mf.loadnd(noise.cuda(), name="noise")
    tv, tf = mf.loadnd(table_dev(shape), name="table")
    sv, sf = mf.framed_1d(rows * 2 * Wh, F32, "cuda", name="scratch")  # exactly n_vol * F * H * 2 * Wh floats
    ov, of = mf.framed_nd(shape, F32, "cuda", name="out")
    for again in (False, True):
        got = ops.free_init_filter(xv, nv, tv, out=ov, scratch=sv)
        torch.cuda.synchronize()
        mf.assert_all_intact(xf, nf, tf, sf, of)
        of.assert_written(want)
        mf.assert_no_poison(sv, "scratch")  # every pair of the half spectrum was produced
        assert torch.isfinite(got).all()    # no poison reached the output
        assert (got.double().cpu() - want).abs().max().item() <= bar_of(e32, dmax)
        assert torch.equal(xv.cpu(), x) and torch.equal(nv.cpu(), noise)  # the inputs are read only
        if not again:
            first = got.clone()
            of.poison()
            sf.poison()
    assert torch.equal(got, first)


# ---------------------------------------------------------------- graph
def test_five_launches_capture_and_replay(cuda):
    shape = (2, 5, 6, 10)
    tab = table_dev(shape)
    x, noise = (t.cuda() for t in inputs(shape))
    rows, Wh = shape[0] * shape[1] * shape[2], shape[3] // 2 + 1
    xs, out = x.clone(), torch.empty_like(x)
    scratch = torch.empty(rows * 2 * Wh, device="cuda")
    ops.free_init_filter(xs, noise, tab, out=out, scratch=scratch)  # loads the kernels
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.free_init_filter(xs, noise, tab, out=out, scratch=scratch)
    for seed in (1, 2):
        x2 = inputs(shape, seed)[0].cuda()
        eager = ops.free_init_filter(x2, noise, tab).clone()
        xs.copy_(x2)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), seed
        assert not torch.equal(eager, ops.free_init_filter(x, noise, tab))


# ---------------------------------------------------------------- DenoiseLoop.reschedule
@pytest.fixture(autouse=True)
def no_graph_left_to_the_cyclic_collector():
    """Whatever a test leaves in a reference cycle is collected here, between tests, never in the
    middle of a later test's stream capture."""
    yield
    gc.collect()


def make_sched(kind):
    if kind == "euler":
        return EulerDiscreteScheduler.from_config(None, timestep_spacing="linspace", beta_schedule="linear")
    return DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)


@pytest.fixture(scope="module")
def pipes(cuda):
    """The tiny synthetic pipelines, built once: text-to-video with DDIM and with Euler, and
    video-to-video (DDIM)."""
    d = {"ddim": AnimateDiffPipeline.from_config("tiny", vae=None),
         "euler": AnimateDiffPipeline.from_config("tiny", vae=None, scheduler=make_sched("euler")),
         "v2v": AnimateDiffVideoToVideoPipeline.from_config("tiny")}
    g = torch.Generator().manual_seed(77)
    d["pe"], d["ne"] = torch.randn((1, 77, 64), generator=g), torch.randn((1, 77, 64), generator=g)
    d["ehs"] = torch.cat([d["ne"], d["pe"]])
    return d


@pytest.mark.parametrize("kind", ["ddim", "euler"])
def test_reschedule_serves_a_shorter_schedule_with_the_same_graph(pipes, kind):
    pipe = pipes[kind]
    unet, sched, ehs = pipe.unet, pipe.scheduler, pipes["ehs"]
    lat = torch.randn(1, 4, 4, 16, 16, generator=torch.Generator().manual_seed(9)).cuda() * sched.init_noise_sigma
    sched.set_timesteps(4)
    loop = DenoiseLoop(unet, sched, lat, ehs, 2.0).prime()
    assert loop.graph is not None, loop.graph_error
    graph, four = loop.graph, loop.run().clone()
    sched.set_timesteps(2)
    assert loop.reschedule(sched.timesteps) is loop and loop.n_steps == 2 and loop.capacity == 4
    with pytest.raises(RuntimeError, match="reset"):
        loop.run(1)  # reschedule alone does not restart
    loop.reset(lat)
    two = loop.run().clone()
    assert loop.graph is graph and loop.issued == 2 and int(loop.step_idx.item()) == 2
    fresh = DenoiseLoop(unet, sched, lat, ehs, 2.0).prime()
    assert torch.equal(two, fresh.run())
    assert not torch.equal(two, four)
    # and back up to the capacity, but not past it
    sched.set_timesteps(4)
    loop.reschedule(sched.timesteps).reset(lat)
    assert torch.equal(loop.run(), four) and loop.graph is graph
    sched.set_timesteps(5)
    with pytest.raises(ValueError, match="reschedule"):
        loop.reschedule(sched.timesteps)


# ---------------------------------------------------------------- pipeline plumbing, bitwise
def by_hand(pipe, ehs, lat, gen, counts, schedule=lambda pipe, n: pipe.scheduler.timesteps, **fi):
    """FreeInit composed from its pieces: per iteration a fresh DenoiseLoop (what a plain call
    builds) over counts[i] steps; between two, add_noise at 999 with the initial latents, one
    randn_tensor draw from gen, ops.free_init_filter."""
    init = lat.clone()
    table = ops.free_init_table(*lat.shape[-3:], fi.get("method", "butterworth"), fi.get("order", 4),
                                fi.get("spatial_stop_frequency", 0.25), fi.get("temporal_stop_frequency", 0.25),
                                device="cuda")
    for i, n in enumerate(counts):
        if i > 0:
            z_t = pipe.scheduler.add_noise(lat, init, torch.full((lat.shape[0],), 999))
            z_rand = P.randn_tensor(lat.shape, generator=gen, device="cuda", dtype=torch.float32)
            lat = ops.free_init_filter(z_t.contiguous(), z_rand, table)
        pipe.scheduler.set_timesteps(n)
        lat = DenoiseLoop(pipe.unet, pipe.scheduler, lat, ehs, 7.5, timesteps=schedule(pipe, n)).prime().run().clone()
    return lat


def t2v_kw(pipes, **more):
    kw = dict(prompt_embeds=pipes["pe"], negative_prompt_embeds=pipes["ne"], num_frames=4, height=128, width=128,
              num_inference_steps=3, guidance_scale=7.5, output_type="latent")
    kw.update(more)
    return kw


def test_pipeline_two_iterations_are_two_plain_calls_around_the_filter(pipes):
    pipe = pipes["ddim"]
    gen = lambda: torch.Generator().manual_seed(21)  # noqa: E731
    off = pipe(**t2v_kw(pipes, generator=gen())).frames.clone()
    pipe.enable_free_init(num_iters=2)
    try:
        assert pipe.free_init_enabled
        on = pipe(**t2v_kw(pipes, generator=gen())).frames.clone()
    finally:
        pipe.disable_free_init()
    # by hand, from plain calls of the pipeline itself
    g = gen()
    first = pipe(**t2v_kw(pipes, generator=g)).frames.clone()      # leaves g after the latents' draw
    assert torch.equal(first, off)
    pipe.scheduler.set_timesteps(3)
    init = pipe.prepare_latents(1, 4, 16, 16, generator=gen())
    z_t = pipe.scheduler.add_noise(first, init, torch.full((1,), 999))
    z_rand = P.randn_tensor(init.shape, generator=g, device="cuda", dtype=torch.float32)
    mixed = ops.free_init_filter(z_t.contiguous(), z_rand, ops.free_init_table(4, 16, 16, device="cuda"))
    want = pipe(**t2v_kw(pipes, latents=mixed)).frames
    assert torch.equal(on, want)
    assert torch.isfinite(on).all() and not torch.equal(on, off)
    # the DenoiseLoop composition the other cases use is the same thing
    assert torch.equal(by_hand(pipe, pipes["ehs"], init, gen_after_latents(gen(), init.shape, pipe), [3, 3]), on)
    # disabled again: the plain result, bit for bit
    assert not pipe.free_init_enabled
    assert torch.equal(pipe(**t2v_kw(pipes, generator=gen())).frames, off)


def gen_after_latents(g, shape, pipe):
    """g after the draw prepare_latents makes of it."""
    P.randn_tensor(shape, generator=g, device="cuda", dtype=pipe.torch_dtype or torch.float32)
    return g


@pytest.mark.parametrize("kind", ["ddim", "euler"])
def test_pipeline_fast_sampling_reschedules_one_loop(pipes, kind, monkeypatch):
    pipe = pipes[kind]
    made = []

    def spy(*a, **k):
        # a function, not a subclass defined here: a class is always part of a reference cycle, and
        # one that reaches a loop would leave the loop's graph to the cyclic collector, which may
        # run inside a later capture (a graph must not be destroyed while a stream is capturing)
        made.append(DenoiseLoop(*a, **k))
        return made[-1]

    fi = dict(num_iters=3, use_fast_sampling=True, method="gaussian", order=2, spatial_stop_frequency=0.3,
              temporal_stop_frequency=0.2)
    # 6 steps: Euler's linspace schedule holds timestep 999, where add_noise looks it up, from 2 steps on
    counts = [R.fast_sampling_steps(6, 3, i) for i in range(3)]
    assert counts == [2, 4, 6]
    pipe.enable_free_init(**fi)
    monkeypatch.setattr(P, "DenoiseLoop", spy)
    try:
        on = pipe(**t2v_kw(pipes, generator=torch.Generator().manual_seed(4), num_inference_steps=6)).frames.clone()
    finally:
        monkeypatch.undo()
        pipe.disable_free_init()
    (loop,) = made  # one loop, one capture, three schedules
    assert loop.capacity == 6 and loop.n_steps == 6 and loop.graph is not None
    g = torch.Generator().manual_seed(4)
    pipe.scheduler.set_timesteps(6)
    init = pipe.prepare_latents(1, 4, 16, 16, generator=g)
    assert torch.equal(by_hand(pipe, pipes["ehs"], init, g, counts, **fi), on)
    # without fast sampling every iteration runs all the steps
    pipe.enable_free_init(num_iters=2)
    try:
        slow = pipe(**t2v_kw(pipes, generator=torch.Generator().manual_seed(4), num_inference_steps=2)).frames.clone()
    finally:
        pipe.disable_free_init()
    g = torch.Generator().manual_seed(4)
    pipe.scheduler.set_timesteps(2)
    init = pipe.prepare_latents(1, 4, 16, 16, generator=g)
    assert torch.equal(by_hand(pipe, pipes["ehs"], init, g, [2, 2]), slow)


def test_video_to_video_cuts_every_iteration_by_strength(pipes):
    pipe = pipes["v2v"]
    video = torch.rand((2, 3, 16, 16), generator=torch.Generator().manual_seed(12))
    kw = dict(video=video, prompt_embeds=pipes["pe"], negative_prompt_embeds=pipes["ne"], guidance_scale=7.5,
              strength=0.6, num_inference_steps=5, output_type="latent")
    off = pipe(generator=torch.Generator().manual_seed(5), **kw).frames.clone()
    pipe.enable_free_init(num_iters=2)
    try:
        on = pipe(generator=torch.Generator().manual_seed(5), **kw).frames.clone()
    finally:
        pipe.disable_free_init()
    g = torch.Generator().manual_seed(5)
    pipe.scheduler.set_timesteps(5)
    ts, n = pipe.get_timesteps(5, 0.6)
    assert n == 3
    init = pipe.prepare_latents(P.preprocess_video(video), ts[:1], generator=g)
    want = by_hand(pipe, pipes["ehs"], init, g, [5, 5], schedule=lambda p, n: p.get_timesteps(n, 0.6)[0])
    assert torch.equal(on, want) and not torch.equal(on, off)
    assert torch.equal(pipe(generator=torch.Generator().manual_seed(5), **kw).frames, off)


def test_free_noise_and_free_init_together(pipes):
    pipe = pipes["ddim"]
    kw = t2v_kw(pipes, num_inference_steps=2)
    kw["num_frames"] = 6
    pipe.enable_free_noise(context_length=4, context_stride=2)
    try:
        pipe.enable_free_init(num_iters=2)
        on = pipe(**kw, generator=torch.Generator().manual_seed(8)).frames.clone()
        pipe.disable_free_init()
        g = torch.Generator().manual_seed(8)
        pipe.scheduler.set_timesteps(2)
        init = pipe.prepare_latents(1, 6, 16, 16, generator=g)  # FreeNoise's rescheduled noise
        assert init.shape == (1, 4, 6, 16, 16)
        assert torch.equal(by_hand(pipe, pipes["ehs"], init, g, [2, 2]), on)
    finally:
        pipe.disable_free_init()
        pipe.disable_free_noise()


def test_frame_sharded_pipeline_is_not_implemented_by_name(pipes):
    pipe = pipes["ddim"]
    pipe.enable_free_init(num_iters=2)
    pipe.dist = object()
    try:
        with pytest.raises(NotImplementedError, match="FreeInit"):
            pipe(**t2v_kw(pipes))
        v2v = pipes["v2v"]
        v2v.enable_free_init()
        v2v.dist = object()
        try:
            with pytest.raises(NotImplementedError, match="FreeInit"):
                v2v(latents=torch.zeros(1, 4, 2, 8, 8), prompt_embeds=pipes["pe"], output_type="latent")
        finally:
            v2v.dist = None
            v2v.disable_free_init()
    finally:
        pipe.dist = None
        pipe.disable_free_init()
    with pytest.raises(NotImplementedError, match="eta"):
        pipe(**t2v_kw(pipes), eta=0.5)
