"""AnimateDiffPipeline-compatible denoising loop on MI355X.

Mirrors the `pipe(...)` surface the reference drives at
experiments/05_grid_search_ablation.py:121-169 (from_pretrained-like
construction, settable `.scheduler`, enable_vae_slicing()/
enable_model_cpu_offload() as no-ops, `pipe(prompt=, negative_prompt=,
num_frames=, guidance_scale=, num_inference_steps=, height=, width=,
generator=).frames[0]`) and the loop body of diffusers'
AnimateDiffPipeline.__call__:

    x_in = cat([x, x]); eps = unet(x_in, t, ehs).sample
    eps = eps_u + g (eps_c - eps_u); x = scheduler.step(eps, t, x).prev_sample

Here that body is ONE captured hipGraph (torch.cuda.CUDAGraph == hipGraph on
ROCm): time embedding from a device timestep table indexed by a device step
counter, the UNet on packed NHWC rows, the fused CFG+DDIM kernel that also
writes the next step's packed input, and the counter increment — replayed
num_inference_steps times with no host work in between.  The cross-attention
K/V of the (constant) prompt embeddings are projected once per video, outside
the graph.

Text encoding: with a `vdiff.CLIPTextModel` and a `vdiff.CLIPTokenizer` (what from_pretrained
loads from a directory's text_encoder/ and tokenizer/) encode_prompt is diffusers': tokenize to
77 ids, one batched encoder forward for the positive and the negative prompts together,
optional clip_skip.  Without a tokenizer the deterministic stub SyntheticTextEncoder stands in
(from_config's synthetic pipelines); embeddings can always be passed as prompt_embeds.
VAE decoding (§8f rank 1) runs when the pipeline holds a `vdiff.AutoencoderKL` (from_config builds one
by default): output_type "pil" (diffusers' default: `.frames[0]` is the first video's
list of PIL images, which 05_grid_search_ablation.py:169-182 saves as PNG / GIF),
"pt" / "np" (diffusers' postprocessed video, (B, F, 3, H, W) tensor / (B, F, H, W, 3)
array in [0, 1]) or "latent" (the final latents).

prepare_latents follows diffusers' randn_tensor: x_T = torch.randn(shape, generator, dtype)
drawn on the generator's device — the CPU for 05:156's `torch.manual_seed(seed)`, the GPU
for 01:103's `torch.Generator("cuda").manual_seed(seed)` — in the pipeline's torch_dtype
(float16 in the reference, 05:35, 05:130-134), then moved to the GPU (kept in fp32 from
there on).

AnimateDiffVideoToVideoPipeline (diffusers' second AnimateDiff pipeline) starts the same loop
from a video: the frames are encoded by the VAE encoder (`AutoencoderKL(..., encoder=True)`),
noised to the timestep `strength` picks, and denoised over the remaining timesteps.

FreeInit (diffusers' FreeInitMixin, `enable_free_init`) wraps the loop of both pipelines: the video
is sampled num_iters times on ONE DenoiseLoop and one captured graph (`DenoiseLoop.reschedule`
swaps in the shorter schedules of use_fast_sampling), and between two runs the latents are noised
back with the initial noise and low-pass mixed with fresh noise by `ops.free_init_filter`.

With a `vdiff.LCMScheduler` the step is stochastic: the pipelines draw the noise of every non-final
step right after the initial latents (diffusers' draw order) and DenoiseLoop keeps it in device
memory behind the coefficient rows, where the step kernel reads it by the device step counter —
still one captured graph.  LoRAs (`load_lora_weights`, `set_adapters`, ... — vdiff.lora) are merged
into the UNet's parameters before the call.

With a `vdiff.DPMSolverMultistepScheduler` (DPM-Solver++ 2M, usually 20-25 steps) the step is
multistep: DenoiseLoop holds the previous step's x0 prediction in `x0_hist`, which the step kernel
reads and overwrites in place, so the state is carried from one graph replay to the next without
host work.  Its SDE type draws one fp32 noise slab per step, kept behind the rows as LCM's are.

With a `vdiff.UniPCMultistepScheduler` (the predictor-corrector solver, usually 10-20 steps) the
step kernel runs the previous step's corrector and this step's predictor in one pass; DenoiseLoop
holds its state — the last two x0 predictions and the sample the previous predictor started from —
in the three slabs of `unipc_state`, read and overwritten in place like `x0_hist`.

With a `vdiff.EulerAncestralDiscreteScheduler` ("Euler a") the Euler step goes down to sigma_down and
adds noise of scale sigma_up: one noise slab per step, drawn up front in diffusers' order and kept
behind the 4-float rows as LCM's are (`VD_STEP_ANCESTRAL` on the Euler step kernel).

AnimateDiffControlNetPipeline (diffusers' third AnimateDiff pipeline) conditions the video on
per-frame control images: a `vdiff.ControlNetModel` runs on the step's input inside the same
captured graph and its 13 residuals are added to the UNet's skips and mid-block output by
`ops.ctrl_add_`, whose scale is read on the device from a [steps][13] table by the step index —
control_guidance_start / end and guess mode change it between replays, not the graph.  The
conditioning embedding depends on no timestep and is computed once per call.

AnimateDiffSparseControlNetPipeline (diffusers' fifth AnimateDiff pipeline, SparseCtrl) conditions
the video on a few key frames: `ops.sparse_cond` (vd_rows_eltwise op 8) builds the condition rows
with their mask column in one launch, a `vdiff.SparseControlNetModel` — the UNet's encoder with its
motion modules, which reads no latents — embeds them once per call and runs inside the captured
graph through the same `control=` path, with one scale for every step.
"""
from __future__ import annotations

import math
import zlib
from collections import namedtuple
from pathlib import Path

import torch

from . import ops
from .models.clip import CLIPTextModel
from .models.controlnet import ControlNetModel, control_scale_table
from .models.sparse_controlnet import SparseControlNetModel
from .models.unet_motion import CIN_PAD, UNetMotionModel
from .models.vae import AutoencoderKL
from .sched.ddim import DDIMScheduler
from .weights import init_synthetic_

AnimateDiffPipelineOutput = namedtuple("AnimateDiffPipelineOutput", ["frames"])


class ControlNetConditioning:
    """What DenoiseLoop(control=) takes: the ControlNet, the conditioning frames (B, 3, F, 8h, 8w)
    fp32 in [0, 1] (one video is shared by the whole batch) and the arguments of diffusers' scale
    rule (vdiff.models.controlnet.control_scale_table)."""

    def __init__(self, controlnet, frames, scale=1.0, guess_mode=False, start=0.0, end=1.0):
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError("a list of ControlNets (MultiControlNetModel) is not supported: pass one")
        self.controlnet, self.frames = controlnet, frames
        self.scale, self.guess_mode, self.start, self.end = scale, bool(guess_mode), start, end

    def table(self, n_steps, n_res):
        return control_scale_table(n_steps, n_res, self.scale, self.guess_mode, self.start, self.end)

    @property
    def reads_latents(self) -> bool:
        """Whether the ControlNet's forward_rows takes the step's latent rows in front of the
        condition rows (SparseControlNetModel reads no latents)."""
        return getattr(self.controlnet, "reads_latents", True)

    def condition_rows(self, B, F, H, W):
        """The rows DenoiseLoop hands to forward_rows at every step, for B videos of F frames of
        H x W latents: computed once, they depend on no timestep."""
        fr = self.frames
        if fr.dim() != 5 or fr.shape[0] not in (1, B) or fr.shape[2] != F or tuple(fr.shape[3:]) != (8 * H, 8 * W):
            raise ValueError(f"conditioning frames of shape {tuple(fr.shape)}: expected (1 or {B}, 3, {F}, "
                             f"{8 * H}, {8 * W})")
        return self.controlnet.embed_condition(fr.expand(B, -1, -1, -1, -1))


class SparseControlConditioning(ControlNetConditioning):
    """DenoiseLoop(control=) for a SparseControlNetModel: the packed condition rows of
    ops.sparse_cond — n_videos (1, shared by the batch, or the batch) videos of `frames` frames of
    h x w condition pixels, the mask in column conditioning_channels — and the scale, which holds
    at every step (diffusers' sparse pipeline has no guidance window); guess mode weighs the
    residuals.  from_tensors takes diffusers' (B, C, F, h, w) condition and (B, 1, F, h, w) mask."""

    def __init__(self, controlnet, cond_rows, n_videos, frames, h, w, scale=1.0, guess_mode=False):
        super().__init__(controlnet, None, scale, guess_mode, 0.0, 1.0)
        if cond_rows.dim() != 2 or tuple(cond_rows.shape) != (n_videos * frames * h * w, CIN_PAD):
            raise ValueError(f"condition rows of shape {tuple(cond_rows.shape)}: expected "
                             f"{(n_videos * frames * h * w, CIN_PAD)}")
        self.cond_rows, self.geometry = cond_rows, (n_videos, frames, h, w)

    @classmethod
    def from_tensors(cls, controlnet, controlnet_cond, conditioning_mask, scale=1.0, guess_mode=False):
        B, _, Fr, h, w = controlnet_cond.shape
        return cls(controlnet, controlnet.condition_rows(controlnet_cond, conditioning_mask), B, Fr, h, w, scale,
                   guess_mode)

    def condition_rows(self, B, F, H, W):
        n, fr, h, w = self.geometry
        ds = self.controlnet.condition_downscale
        if n not in (1, B) or fr != F or (h, w) != (ds * H, ds * W):
            raise ValueError(f"sparse condition of {n} videos x {fr} frames x {h} x {w}: expected 1 or {B} videos x "
                             f"{F} frames x {ds * H} x {ds * W}")
        emb = self.controlnet.embed_condition(self.cond_rows, n * F, h, w)
        return emb if n == B else emb.repeat(B, 1)


class ControlState:
    """One step's ControlNet residuals and where their scales live: UNetMotionModel.forward_rows
    calls inject() after the mid block.  cond_only (guess mode under CFG): the residuals are the
    conditional half's and touch that half's rows alone."""

    def __init__(self, residuals, block, cond_only):
        self.residuals, self.block, self.cond_only = residuals, block, cond_only

    def inject(self, skips, mid, ctx):
        accs = [*skips, mid]
        if len(accs) != len(self.residuals):
            raise ValueError(f"{len(self.residuals)} ControlNet residuals for the UNet's {len(accs) - 1} skips + mid")
        for i, (a, r) in enumerate(zip(accs, self.residuals)):
            acc = a.t[a.t.shape[0] // 2:] if self.cond_only else a.t
            ops.ctrl_add_(acc, r.t, self.block, i, cols=len(accs))


class SyntheticTextEncoder:
    """Stand-in for CLIPTextModel where no tokenizer / weights are given (synthetic
    pipelines): prompt -> deterministic N(0,1) [77, dim] embedding seeded by crc32(prompt)."""

    def __init__(self, dim: int, seq_len: int = 77):
        self.dim, self.seq_len = dim, seq_len

    def __call__(self, prompt: str) -> torch.Tensor:
        g = torch.Generator().manual_seed(zlib.crc32(prompt.encode()))
        return torch.randn((self.seq_len, self.dim), generator=g)


class PerturbedAttentionGuidance:
    """The two numbers of diffusers' PAGMixin: pag_scale and pag_adaptive_scale.  scale_at(t) is
    its _get_pag_scale — max(pag_scale - pag_adaptive_scale * (1000 - t), 0) under adaptive scaling
    (pag_adaptive_scale > 0), else pag_scale — evaluated in fp64 and rounded to fp32 once, in the
    device table (diffusers evaluates it on the step's timestep tensor)."""

    def __init__(self, scale: float = 3.0, adaptive_scale: float = 0.0):
        self.scale, self.adaptive_scale = float(scale), float(adaptive_scale)
        if not (math.isfinite(self.scale) and self.scale > 0) or not (math.isfinite(self.adaptive_scale)
                                                                      and self.adaptive_scale >= 0):
            raise ValueError(f"PAG needs pag_scale > 0 and pag_adaptive_scale >= 0, got {scale!r}, {adaptive_scale!r}")

    def scale_at(self, t) -> float:
        if self.adaptive_scale > 0:
            return max(self.scale - self.adaptive_scale * (1000 - float(t)), 0.0)
        return self.scale

    def table(self, timesteps):
        return [self.scale_at(t) for t in torch.as_tensor(timesteps).tolist()]


class DenoiseLoop:
    """Preallocated device state + the captured graph of one denoising step."""

    def __init__(self, unet: UNetMotionModel, scheduler, latents: torch.Tensor,
                 prompt_embeds: torch.Tensor, guidance_scale: float, timesteps=None,
                 use_graph: bool = True, cfg_shard=None, ip_embeds=None, step_noise=None, control=None, pag=None):
        """step_noise (a stochastic scheduler only, where it is required): the noise of the
        stochastic steps in step order.  LCM: [n_steps - 1 or n_steps, B, C, F, H, W] (the last
        step adds none; a row given for it is ignored).  The SDE type of
        DPMSolverMultistepScheduler and EulerAncestralDiscreteScheduler: [n_steps, B, C, F, H, W], one
        slab per step (Euler ancestral's last step reads none: its sigma_up is 0).  It lives
        behind the coefficient rows in one device buffer that the step kernel reads by the device
        step index, so the captured graph serves any later reset(latents, step_noise=...).
        ip_embeds: the projected IP-Adapter image tokens [Bt, n, cross_attention_dim] (uncond
        half first under CFG), or None.  They become n extra K/V rows per video in every spatial
        cross-attention (built once, in prime()'s eager step) and the attention launches take
        them as a second softmax segment; not supported together with cfg_shard.
        control (ControlNetConditioning): the ControlNet runs on the step's input before the UNet
        (on the conditional half alone in guess mode under CFG) with a Ctx and a cross-attention
        K/V cache of its own, and its residuals are added after the UNet's mid block, scaled by the
        [capacity][n] table behind the control block's header — whose first word is this loop's
        device step counter.  Not supported under frame or CFG sharding.
        pag (PerturbedAttentionGuidance): perturbed-attention guidance.  The UNet batch gains one
        branch, the LAST one, in which the self-attentions marked by
        unet.set_pag_applied_layers(...) use an identity attention map: 3 branches
        [uncond; cond; perturbed] under CFG, 2 branches [cond; perturbed] without.  prompt_embeds
        (and ip_embeds) hold one entry per branch, the perturbed one the conditional embeddings
        again: [neg, pos, pos] or [pos, pos].  The step kernel combines the branches
        (VD_STEP_PAG) with the step's PAG scale, which it reads by the device step index from the
        table in front of coef, so adaptive scaling replays on the one captured graph.  Not
        supported with cfg_shard, frame sharding, FreeNoise or ControlNet.
        cfg_shard (vdiff.dist.CfgShard, CFG only): this rank runs the UNet on ONE half
        (cfg_shard.index: 0 uncond, 1 cond) and swaps eps rows with its pair before the
        fused CFG+scheduler update, which both ranks apply to their replicated latents
        (SURVEY.md §8e (ii)).  prompt_embeds still holds both halves, uncond first.
        prompt_embeds: [Bt, L, D], Bt the guidance branches times the videos, or the per-frame form
        [Bt * F, L, D] (FreeNoise prompt travel, AnimateDiffPipeline.encode_prompt_free_noise): rows
        (branch, video, frame), every frame's spatial cross-attention reads its own text.  The K/V
        cache is still filled once per loop and is F times larger.  Not supported with ip_embeds,
        cfg_shard, pag or frame sharding, whose text row layouts are per video."""
        n_br = (2 if guidance_scale > 1 else 1) + (pag is not None)
        if latents.shape[2] > 1 and prompt_embeds.shape[0] == n_br * latents.shape[0] * latents.shape[2]:
            what = ("ip_embeds (IP-Adapter)" if ip_embeds is not None else "cfg_shard" if cfg_shard is not None else
                    "perturbed-attention guidance (pag=)" if pag is not None else
                    "frame sharding (dist=)" if getattr(unet, "dist", None) is not None else None)
            if what is not None:  # before any device work
                raise NotImplementedError(f"per-frame text (prompt travel) together with {what} is not supported: "
                                          "the text + image K/V rows and the sharded text rows are laid out per video")
        if not unet._prepared:
            unet.prepare()
        dev = unet.device
        self.unet = unet
        # guidance branches through the UNet: the CFG pair or the one conditional pass, and PAG's
        # perturbed branch behind them
        n_cfg = 2 if guidance_scale > 1 else 1
        self.pag = pag
        if pag is not None:
            what = ("cfg_shard" if cfg_shard is not None else "frame sharding (dist=)" if unet.dist is not None else
                    "FreeNoise" if unet.free_noise_enabled else "ControlNet" if control is not None else None)
            if what is not None:
                raise NotImplementedError(f"perturbed-attention guidance with {what} is not supported: the "
                                          "perturbed branch is whole videos at the end of one rank's UNet batch")
            if not unet.pag_applied_layers():
                raise ValueError("DenoiseLoop(pag=...): no self-attention is marked; call "
                                 "unet.set_pag_applied_layers(...) first")
        self.ncfg = n_cfg + (pag is not None)
        self.g = float(guidance_scale)
        self.lat = latents.to(dev, torch.float32).contiguous().clone()
        self.B, _, self.F, self.H, self.W = self.lat.shape
        self.Bt = self.ncfg * self.B
        self.cfg_shard = cfg_shard if n_cfg == 2 else None
        ts = scheduler.timesteps if timesteps is None else timesteps
        self.scheduler = scheduler
        self.n_steps = len(ts)
        self.capacity = len(ts)  # rows of the device tables: the longest schedule reschedule() takes
        self.ts = torch.as_tensor(ts).to(dev, torch.float32)
        # the scheduler's fused CFG+update kernel; Euler's also applies the next step's
        # scale_model_input, and the first input is packed with step 0's divisor
        self.kind = getattr(scheduler, "kind", "ddim")
        self.sched_step = ops.SCHED_STEP[self.kind]
        rows = scheduler.coefficient_table(torch.as_tensor(ts).cpu())
        # the SDE type of DPMSolverMultistepScheduler adds noise on EVERY step, LCM on all but the last
        self.dpm_sde = self.kind == "dpm" and scheduler.sde
        if self.kind == "lcm":
            # one buffer, built once at the loop's capacity: the rows, then one noise slab per row
            if step_noise is None:
                raise ValueError("an LCM DenoiseLoop needs step_noise: the noise of its stochastic steps, "
                                 f"[{self.n_steps - 1} or {self.n_steps}, {', '.join(map(str, self.lat.shape))}]")
            self.coef = torch.empty(ops.lcm_buffer_numel(self.capacity, self.lat.numel()), device=dev,
                                    dtype=torch.float32)
            self.coef_rows = self.coef[:ops.LCM_ROW * self.capacity].view(self.capacity, ops.LCM_ROW)
            self.noise_slabs = self.coef[ops.LCM_ROW * self.capacity:].view(self.capacity, *self.lat.shape)
            self.noise_slabs.zero_()  # the last step's slab is never read; keep it defined all the same
            self.coef_rows.copy_(rows)
            self._fill_step_noise(step_noise)
        elif self.dpm_sde:
            # LCM's layout; every slab is read, the last step's too (times a zero coefficient)
            if step_noise is None:
                raise ValueError("a DenoiseLoop of the SDE type of DPMSolverMultistepScheduler needs step_noise: one "
                                 f"slab per step, [{self.n_steps}, {', '.join(map(str, self.lat.shape))}]")
            self.coef = torch.empty(ops.dpm_buffer_numel(self.capacity, self.lat.numel(), True), device=dev,
                                    dtype=torch.float32)
            self.coef_rows = self.coef[:ops.DPM_ROW * self.capacity].view(self.capacity, ops.DPM_ROW)
            self.noise_slabs = self.coef[ops.DPM_ROW * self.capacity:].view(self.capacity, *self.lat.shape)
            self.noise_slabs.zero_()
            self.coef_rows.copy_(rows)
            self._fill_step_noise(step_noise)
        elif self.kind == "euler_a":
            # LCM's layout behind rows of 4; a slab is read unless its row's sigma_up is 0 (the last step's)
            if step_noise is None:
                raise ValueError("an Euler-ancestral DenoiseLoop needs step_noise: the noise of its stochastic "
                                 f"steps, [{self.n_steps}, {', '.join(map(str, self.lat.shape))}]")
            self.coef = torch.empty(ops.euler_a_buffer_numel(self.capacity, self.lat.numel()), device=dev,
                                    dtype=torch.float32)
            self.coef_rows = self.coef[:ops.EULER_A_ROW * self.capacity].view(self.capacity, ops.EULER_A_ROW)
            self.noise_slabs = self.coef[ops.EULER_A_ROW * self.capacity:].view(self.capacity, *self.lat.shape)
            self.noise_slabs.zero_()
            self.coef_rows.copy_(rows)
            self._fill_step_noise(step_noise)
        else:
            if step_noise is not None:
                raise ValueError("step_noise is for an LCM scheduler or the SDE type of DPMSolverMultistepScheduler; "
                                 f"this loop's is {self.kind!r}")
            self.coef = self.coef_rows = rows.to(dev)
        # a multistep scheduler's state between two replays: the previous step's x0 prediction, which
        # the step kernel reads and overwrites in place.  Step 0 of a schedule never reads it, so
        # neither reset() nor reschedule() clears it.
        self.step_kwargs = {}
        if self.kind == "dpm":
            self.x0_hist = torch.empty_like(self.lat)
            self.step_kwargs = dict(x0_out=self.x0_hist)
        elif self.kind == "unipc":
            # UniPC's: the last two x0 predictions and the sample the previous predictor started from
            self.unipc_state = torch.empty((3,) + tuple(self.lat.shape), device=dev, dtype=torch.float32)
            self.step_kwargs = dict(x0_out=self.unipc_state)
        if pag is not None:
            # the same buffer with the PAG scales in front (ops.pag_coef): re-point the views
            width = self.coef_rows.shape[1]
            self.coef = ops.pag_coef(pag.table(ts), self.coef)
            body = self.coef[ops.pag_prefix(self.capacity):]
            self.pag_tab = self.coef[:self.capacity]
            self.coef_rows = body[:width * self.capacity].view(self.capacity, width)
            if hasattr(self, "noise_slabs"):
                self.noise_slabs = body[width * self.capacity:].view(self.capacity, *self.lat.shape)
            self.step_kwargs["pag_n"] = self.capacity
        self.in_div0 = 1.0
        if self.kind in ("euler", "euler_a"):
            self.in_div0 = scheduler.input_divisor(scheduler.index_for_timestep(float(torch.as_tensor(ts)[0])))
        self.step_idx = torch.zeros(1, device=dev, dtype=torch.int32)
        self.control = control
        if control is not None:
            if cfg_shard is not None or unet.dist is not None:
                raise NotImplementedError("ControlNet under frame sharding (dist=) or CFG sharding (cfg_shard=) is "
                                          "not supported: the residuals are not sharded over the ranks")
            cn = control.controlnet
            if not control.reads_latents and unet.free_noise_enabled:
                raise NotImplementedError("FreeNoise with a SparseControlNetModel is not supported: the ControlNet's "
                                          "own motion modules would need the windows too; disable_free_noise()")
            if not cn._prepared:
                cn.prepare()
            self.cn_res = cn.num_residuals
            want = unet.control_residual_shapes(1, self.H, self.W)
            if [c for _, c in want] != cn.residual_channels() or \
                    cn.time_proj.num_channels != unet.time_proj.num_channels:
                raise ValueError(f"the ControlNet's residual channels {cn.residual_channels()} do not fit the UNet's "
                                 f"skips {[c for _, c in want]}")
            # the step counter moves into the control block's header (ops.ctrl_block)
            self.ctrl_block, self.step_idx = ops.ctrl_block(control.table(self.capacity, self.cn_res), dev)
        pe = prompt_embeds.to(dev, torch.bfloat16).contiguous()
        if pe.shape[0] not in (self.Bt, self.Bt * self.F):
            raise ValueError(f"prompt_embeds batch {pe.shape[0]} != {self.Bt} (uncond first when CFG; with pag= the "
                             f"conditional embeddings once more at the end), or {self.Bt * self.F} in the per-frame "
                             "form (FreeNoise prompt travel: video-major, then frame)")
        self.L = pe.shape[1]
        # per-frame text (FreeNoise prompt travel): F text entries per video, so F times the K/V rows
        # in the cross-attention cache, still projected once per loop
        self.text_frames = self.F if pe.shape[0] != self.Bt else 1
        # the UNet batch: both CFG halves, or this rank's half under cfg_shard
        self.Bu = self.Bt
        if self.cfg_shard is not None:
            h = self.cfg_shard.index
            pe = pe[h * self.B:(h + 1) * self.B].contiguous()
            self.Bu = self.B
        self.ehs_rows = pe.reshape(self.Bu * self.text_frames * self.L, -1)
        self.ip_rows = None
        if ip_embeds is not None:
            if self.cfg_shard is not None:
                raise NotImplementedError("ip_embeds together with cfg_shard is not supported")
            if not unet.has_ip_adapter:
                raise ValueError("ip_embeds given, but the UNet has no IP-Adapter loaded")
            ip = ip_embeds.to(dev, torch.bfloat16).contiguous()
            if ip.dim() != 3 or ip.shape[0] != self.Bt or ip.shape[2] != pe.shape[-1] or not 1 <= ip.shape[1] <= 64:
                raise ValueError(f"ip_embeds of shape {tuple(ip.shape)}: expected [{self.Bt}, n <= 64, {pe.shape[-1]}] "
                                 "(uncond first when CFG)")
            self.ip_rows = ip.reshape(self.Bt * ip.shape[1], -1)
        # the CFG step kernel writes the next input for both halves; under cfg_shard the
        # UNet reads only the first copy (the latents are replicated over the pair)
        self.x_in2 = ops.pack_latents(self.lat, dup=self.ncfg, cpad=CIN_PAD, in_div=self.in_div0)
        self.x_in = self.x_in2[:self.Bu * self.F * self.H * self.W]
        self.kv_cache = {}
        if control is not None:
            cond = control.condition_rows(self.B, self.F, self.H, self.W)
            # guess mode under CFG: the ControlNet sees the conditional half only
            self.cn_cond_only = control.guess_mode and self.ncfg == 2
            self.cn_batch = self.B if self.cn_cond_only else self.Bt
            half = self.B * self.F * self.H * self.W
            self.cn_cond_rows = cond if self.cn_batch == self.B else torch.cat([cond, cond])
            self.cn_x_in = self.x_in[half:] if self.cn_cond_only else self.x_in
            self.cn_ehs_rows = (self.ehs_rows[self.B * self.text_frames * self.L:] if self.cn_cond_only
                                else self.ehs_rows)
            self.cn_kv_cache = {}
        # the FreeU scalars the step's launches (and the graph) read: kept alive for this loop's
        # life, whatever enable_freeu / disable_freeu does to the blocks afterwards
        self.freeu_operands = [b._freeu for b in unet.up_blocks]
        # likewise FreeNoise's window weights (enable_free_noise / disable_free_noise)
        self.free_noise_operands = [m._fn_wt for m in unet.motion_modules_in_order()]
        # conv_in + down_blocks[0].resnets[0] once for both CFG halves (UNetMotionModel.forward_rows)
        self.cfg_dedup = True
        self.use_graph = use_graph
        self.graph = None
        self.graph_error = None
        self.issued = 0  # steps run since the last reset(): the device index into ts / coef

    def _claim(self, n):
        """Host-side bound on the device step counter: the timestep and coefficient tables
        hold n_steps rows; running past them without reset() is an error (the kernels also
        clamp the index, so a stray replay can never read past the tables)."""
        if n < 0 or self.issued + n > self.n_steps:
            raise RuntimeError(f"run({n}) after {self.issued} of {self.n_steps} scheduled steps: "
                               "call reset(latents) to start a new schedule")
        self.issued += n

    def step(self):
        u = self.unet
        te = ops.timestep_embed(self.ts, u.time_proj.num_channels, step_idx=self.step_idx, batch=self.Bu)
        ctx = u.make_ctx(te, self.ehs_rows, self.Bu, self.F, self.L, kv_cache=self.kv_cache, ip_rows=self.ip_rows,
                         pag_batch=self.B if self.pag is not None else 0)
        # x_in = [lat; lat]; not under PAG, whose last branch differs from the first self-attention on
        ctx.cfg_dup = self.cfg_dedup and self.Bu == self.Bt == 2 * self.B and self.pag is None
        state = None
        if self.control is not None:  # every row of te is the step's one timestep
            cn = self.control.controlnet
            cctx = cn.make_ctx(te[:self.cn_batch], self.cn_ehs_rows, self.cn_batch, self.F, self.L,
                               kv_cache=self.cn_kv_cache)
            if self.control.reads_latents:
                res = cn.forward_rows(self.cn_x_in, self.cn_cond_rows, self.H, self.W, cctx)
            else:  # SparseCtrl: timestep, text and condition only
                res = cn.forward_rows(self.cn_cond_rows, self.H, self.W, cctx)
            state = ControlState(res, self.ctrl_block, self.cn_cond_only)
        eps = u.forward_rows(self.x_in, self.H, self.W, ctx, control=state)
        if self.cfg_shard is not None:
            eps = self.cfg_shard.gather_eps(eps)
        self.sched_step(eps, self.ncfg, self.g, self.lat, self.coef, step_idx=self.step_idx,
                        next_in=self.x_in2, **self.step_kwargs)
        ops.step_advance(self.step_idx)

    def _fill_step_noise(self, step_noise):
        """Copy the schedule's step noise into the slabs behind the coefficient rows."""
        want = tuple(self.lat.shape)
        sn = torch.as_tensor(step_noise)
        # one slab per step for the SDE type of DPM and for Euler ancestral, whose draw order has one per step
        counts = (self.n_steps,) if self.dpm_sde or self.kind == "euler_a" else (self.n_steps - 1, self.n_steps)
        if sn.dim() != 6 or tuple(sn.shape[1:]) != want or sn.shape[0] not in counts:
            raise ValueError(f"step_noise of shape {tuple(sn.shape)}: expected [{' or '.join(map(str, counts))}, "
                             f"{', '.join(map(str, want))}] (one slab per stochastic step, in step order)")
        self.noise_slabs[:sn.shape[0]].copy_(sn)

    def reset(self, latents, step_noise=None):
        """Back to step 0 with new latents; a loop with step noise (LCM, the SDE type of
        DPMSolverMultistepScheduler, Euler ancestral) also takes the new run's step_noise (None keeps the slabs it
        holds).  A multistep loop's history needs no clearing: step 0 never reads it."""
        if step_noise is not None:
            if self.kind not in ("lcm", "euler_a") and not self.dpm_sde:
                raise ValueError("step_noise is for an LCM scheduler or the SDE type of DPMSolverMultistepScheduler; "
                                 f"this loop's is {self.kind!r}")
            self._fill_step_noise(step_noise)
        self.lat.copy_(latents)
        self.step_idx.zero_()
        self.issued = 0
        ops.pack_latents(self.lat, dup=self.ncfg, cpad=CIN_PAD, out=self.x_in2, in_div=self.in_div0)

    def reschedule(self, timesteps):
        """Switch to another schedule of at most `capacity` steps without a new capture: its
        timesteps and coefficient rows go into the prefix of the same device tables, which the
        step's launches (and so the captured graph) read by pointer at the device step index.
        scheduler.set_timesteps must already hold the schedule the timesteps come from (Euler's
        coefficients are looked up in it).  reset(latents) must follow before the next run()."""
        ts = torch.as_tensor(timesteps)
        n = len(ts)
        if n < 1 or n > self.capacity:
            raise ValueError(f"reschedule: {n} timesteps, the loop's tables were built for 1..{self.capacity}")
        self.ts[:n].copy_(ts.to(self.ts.device, torch.float32))
        self.coef_rows[:n].copy_(self.scheduler.coefficient_table(ts.cpu()).to(self.coef.device))
        if self.kind in ("euler", "euler_a"):
            self.in_div0 = self.scheduler.input_divisor(self.scheduler.index_for_timestep(float(ts[0])))
        if self.pag is not None:  # the new timesteps' PAG scales
            self.pag_tab[:n].copy_(ops.pag_scales(self.pag.table(ts)))
        if self.control is not None:  # the new schedule's scales, by its own step count
            ops.ctrl_table(self.ctrl_block, self.cn_res)[:n].copy_(self.control.table(n, self.cn_res))
        self.n_steps = n
        self.issued = n  # nothing may run before reset()
        return self

    def prime(self):
        """One eager step (loads kernels, fills the cross-attention K/V cache,
        initialises communicators), then restore the state; capture the graph."""
        saved = self.lat.clone()
        self.step()
        self.reset(saved)
        torch.cuda.synchronize()
        if self.use_graph and self.graph is None:
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self.step()
                self.graph = g
            except Exception as e:  # capture unsupported (e.g. a collective): run eagerly
                self.graph_error = repr(e)
                self.graph = None
                torch.cuda.synchronize()
                self.reset(saved)
        return self

    def run(self, n=None):
        n = self.n_steps - self.issued if n is None else n
        self._claim(n)
        for _ in range(n):
            if self.graph is not None:
                self.graph.replay()
            else:
                self.step()
        return self.lat


def randn_tensor(shape, generator=None, device=None, dtype=None):
    """diffusers.utils.torch_utils.randn_tensor: N(0, 1) drawn on the generator's device (the
    target device when there is no generator), in `dtype`, then moved to `device`.  A list of
    generators draws one batch row each.  A CUDA generator for a CPU target is refused."""
    device = torch.device(device or "cpu")
    gens = generator if isinstance(generator, (list, tuple)) else None
    if gens is not None and len(gens) == 1:
        generator, gens = gens[0], None
    rand_device = device
    if generator is not None:
        gtype = (gens[0] if gens is not None else generator).device.type
        if gtype != device.type:
            if gtype != "cpu":
                raise ValueError(f"Cannot generate a {device} tensor from a generator of type {gtype}.")
            rand_device = torch.device("cpu")
    if gens is not None:
        if len(gens) != shape[0]:
            raise ValueError(f"{len(gens)} generators for a batch of {shape[0]}")
        one = (1,) + tuple(shape[1:])
        x = torch.cat([torch.randn(one, generator=gen, device=rand_device, dtype=dtype) for gen in gens])
    else:
        x = torch.randn(shape, generator=generator, device=rand_device, dtype=dtype)
    return x.to(device)


def numpy_to_pil(images):
    """diffusers' numpy_to_pil: (F, H, W, 3) floats in [0, 1] -> list of RGB PIL images."""
    from PIL import Image
    arr = (images * 255).round().astype("uint8")
    return [Image.fromarray(a) for a in arr]


def export_to_gif(frames, output_gif_path, fps: int = 10):
    """diffusers.utils.export_to_gif (05:28, :181): PIL frames -> an animated GIF."""
    frames[0].save(str(output_gif_path), save_all=True, append_images=list(frames[1:]), optimize=False,
                   duration=1000 // fps, loop=0)
    return str(output_gif_path)


class AnimateDiffPipeline:
    # dtype the initial noise is drawn in on the CPU generator: the reference loads the
    # pipeline with torch_dtype=torch.float16 (05:35, 05:130-134) and diffusers' randn_tensor
    # draws in that dtype
    latent_draw_dtype = torch.float16
    vae_encoder = False  # from_config's synthetic VAE: decoder only (text-to-video never encodes)

    def __init__(self, unet: UNetMotionModel, scheduler=None, text_encoder=None, vae=None, dist=None,
                 tokenizer=None):
        self.unet = unet
        self.scheduler = scheduler or DDIMScheduler()
        self.text_encoder = text_encoder or SyntheticTextEncoder(unet.config["cross_attention_dim"])
        self.tokenizer = tokenizer
        if tokenizer is not None and not isinstance(self.text_encoder, CLIPTextModel):
            raise ValueError("tokenizer= needs text_encoder=vdiff.CLIPTextModel(...)")
        self.vae = vae
        self.dist = dist
        self.unet.dist = dist
        # IP-Adapter (load_ip_adapter): the CLIP vision tower, its preprocessing, the projection
        self.image_encoder = None
        self.feature_extractor = None
        self.image_projection = None
        self._free_noise = None  # (context_length, context_stride, noise_type) while FreeNoise is enabled
        self._free_init_num_iters = None  # enable_free_init's arguments while FreeInit is enabled
        # the dtype the initial noise is drawn in (diffusers: prompt_embeds.dtype, i.e. the
        # pipeline's torch_dtype, fp32 when none is given); from_config keeps the reference's fp16
        self.torch_dtype = None

    @classmethod
    def from_config(cls, config="full", device="cuda", seed=0, scheduler=None, dist=None, vae="auto"):
        """Synthetic-weight pipeline; vae "auto" (a synthetic AutoencoderKL of the UNet's config,
        so the default output_type "pil" works), "tiny"/"full", an AutoencoderKL instance, or
        None (latents only)."""
        if vae == "auto":
            vae = config if config in ("tiny", "full") else None
        unet = UNetMotionModel(config)
        init_synthetic_(unet, seed)
        unet = unet.to(device=device, dtype=torch.bfloat16)
        unet.prepare()
        sched = scheduler or DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1,
                                                       clip_sample=False)
        if isinstance(vae, str):
            vae = init_synthetic_(AutoencoderKL(vae, encoder=cls.vae_encoder), seed).to(device=device, dtype=torch.bfloat16).prepare()
        pipe = cls(unet, sched, dist=dist, vae=vae)
        pipe.torch_dtype = cls.latent_draw_dtype  # the reference's torch_dtype=torch.float16 (05:35)
        return pipe

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, motion_adapter=None, torch_dtype=None, variant=None,
                        device="cuda", dist=None, **unused):
        """diffusers AnimateDiffPipeline.from_pretrained(path, motion_adapter=, torch_dtype=) as
        05:130-134 calls it, over a LOCAL diffusers-layout directory (vdiff.pretrained): unet/
        joined with the MotionAdapter's motion modules, vae/ (decoder), scheduler/, and — when
        BOTH exist — text_encoder/ (vdiff.CLIPTextModel) with tokenizer/ (vdiff.CLIPTokenizer).
        Without the two the text encoder stays the deterministic stub (pass prompt_embeds for
        real embeddings).  device="cpu" builds the modules without preparing device operands."""
        from . import pretrained as P
        root = P._local_dir(pretrained_model_name_or_path, "AnimateDiffPipeline.from_pretrained")
        if motion_adapter is None:
            raise ValueError("AnimateDiffPipeline needs motion_adapter=MotionAdapter.from_pretrained(...)")
        unet = P.load_unet_motion(root / "unet", motion_adapter, device=device, variant=variant)
        vae = P.load_vae(root / "vae", device=device, variant=variant) if (root / "vae").is_dir() else None
        sched = P.load_scheduler(root / "scheduler") if (root / "scheduler").is_dir() else None
        enc = tok = None
        if (root / "text_encoder").is_dir() and (root / "tokenizer").is_dir():
            enc = P.load_text_encoder(root / "text_encoder", device=device, variant=variant)
            tok = P.load_tokenizer(root / "tokenizer")
        if torch.device(device).type == "cuda":
            unet.prepare()
            if vae is not None:
                vae.prepare()
            if enc is not None:
                enc.prepare()
        pipe = cls(unet, sched, text_encoder=enc, dist=dist, vae=vae, tokenizer=tok)
        pipe.torch_dtype = torch_dtype
        return pipe

    def enable_vae_slicing(self):
        pass  # decoding is always chunked (AutoencoderKL.frames_per_chunk)

    def enable_model_cpu_offload(self, *a, **k):
        pass  # 288 GB HBM: the 12 GB-GPU workaround is unnecessary

    def to(self, *a, **k):
        return self

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """diffusers' FreeUMixin.enable_freeu (UNetMotionModel.enable_freeu); the next __call__
        builds its DenoiseLoop, and so its graph, with it."""
        self.unet.enable_freeu(s1=s1, s2=s2, b1=b1, b2=b2)

    def disable_freeu(self):
        self.unet.disable_freeu()

    # ------------------------------------------------------------------ LoRA
    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, weight_name=None, subfolder=None,
                          adapter_name=None, **unused):
        """diffusers' load_lora_weights over LOCAL files (vdiff.lora): a state dict, a .safetensors /
        .bin file, or a directory (+ subfolder, weight_name).  The LoRA is merged into the UNet's
        parameters as a new active adapter of weight 1.0 (the adapters already active stay active)
        and the operands are re-packed.  Like enable_freeu it acts on the next __call__, which
        builds its DenoiseLoop — graph and cross-attention K/V cache included — from scratch."""
        from . import lora
        sd = lora.read_lora_file(pretrained_model_name_or_path_or_dict, weight_name=weight_name, subfolder=subfolder)
        return self.unet.load_lora_state_dict(sd, adapter_name=adapter_name)

    def set_adapters(self, adapter_names, adapter_weights=None):
        """The active adapters and their weights (default 1.0 each); weight 0 is the base weight."""
        self.unet.set_adapters(adapter_names, adapter_weights)

    def get_active_adapters(self):
        return self.unet.get_active_adapters()

    def delete_adapters(self, adapter_names):
        self.unet.delete_adapters(adapter_names)

    def unload_lora_weights(self):
        """Every UNet parameter back to its base tensor, bit for bit."""
        self.unet.unload_lora()

    def fuse_lora(self, lora_scale: float = 1.0, **unused):
        """Accepted for diffusers' call sequence: the weights here are always merged, so this only
        multiplies the active adapters' weights by lora_scale."""
        from . import lora
        lora.set_fuse_scale(self.unet, lora_scale)

    def unfuse_lora(self, **unused):
        from . import lora
        lora.set_fuse_scale(self.unet, 1.0)

    # ------------------------------------------------------------------ FreeNoise
    FREE_NOISE_NOISE_TYPES = ("shuffle_context", "repeat_context", "random")

    def enable_free_noise(self, context_length=16, context_stride=4, weighting_scheme="pyramid",
                          noise_type="shuffle_context", prompt_interpolation_callback=None):
        """diffusers' AnimateDiffFreeNoiseMixin.enable_free_noise: the motion modules run on sliding
        windows (UNetMotionModel.enable_free_noise) and the text-to-video pipeline reschedules its
        initial noise (_prepare_latents_free_noise), so num_frames may exceed
        motion_max_seq_length.  The next __call__ builds its DenoiseLoop, and so its graph, with it."""
        if noise_type not in self.FREE_NOISE_NOISE_TYPES:
            raise ValueError(f"noise_type {noise_type!r}: one of {self.FREE_NOISE_NOISE_TYPES}")
        if prompt_interpolation_callback is not None:
            raise NotImplementedError("a custom prompt_interpolation_callback is not supported: FreeNoise prompt "
                                      "travel (a {frame: text} prompt) interpolates linearly, diffusers' default, "
                                      "on the device (vd_rows_eltwise op 9)")
        self.unet.enable_free_noise(context_length, context_stride, weighting_scheme)
        m = self.unet.motion_modules_in_order()[0]
        self._free_noise = (m.context_length, m.context_stride, noise_type)

    def disable_free_noise(self):
        self._free_noise = None
        self.unet.disable_free_noise()

    @property
    def free_noise_enabled(self) -> bool:
        return getattr(self, "_free_noise", None) is not None

    def enable_free_noise_split_inference(self, spatial_split_size=256, temporal_split_size=16):
        raise NotImplementedError("enable_free_noise_split_inference (diffusers' SplitInferenceModule memory "
                                  "splitting) is not supported: the windows run as one batch")

    def _prepare_latents_free_noise(self, batch, num_frames, h, w, generator=None, latents=None, device=None):
        """diffusers' AnimateDiffFreeNoiseMixin._prepare_latents_free_noise, in pure torch (runs on
        the CPU with a CPU generator): noise over num_frames frames in which distant windows see
        correlated noise, before init_noise_sigma.
          shuffle_context  all num_frames frames are drawn; then for i in range(L, F, s) frames
                           i .. i + s take frames i - L .. i - L + s in a randperm order drawn from
                           the same generator on its device (a prefix when they do not fit);
          repeat_context   L frames are drawn and tiled;
          random           as drawn.
        `latents` with num_frames frames pass through unchanged; with L frames they are tiled to
        num_frames and, under shuffle_context, shuffled as above; any other length is refused."""
        L, s, noise_type = self._free_noise
        device = torch.device(device if device is not None else self.unet.device)
        dtype = self.torch_dtype or torch.float32
        C = self.unet.config["in_channels"]
        if latents is None:
            draw = L if noise_type == "repeat_context" else num_frames
            latents = randn_tensor((batch, C, draw, h, w), generator=generator, device=device, dtype=dtype)
            if noise_type == "random":
                return latents
        else:
            if latents.shape[2] == num_frames:
                return latents.to(device)
            if latents.shape[2] != L:
                raise ValueError(f"latents hold {latents.shape[2]} frames: FreeNoise takes num_frames={num_frames} "
                                 f"or context_length={L}")
            latents = latents.to(device)
        if latents.shape[2] < num_frames:  # repeat_context, or L user frames: tile
            latents = torch.cat([latents] * (-(-num_frames // L)), dim=2)[:, :, :num_frames].contiguous()
        if noise_type == "shuffle_context":
            gens = generator if isinstance(generator, (list, tuple)) else [generator]
            g0 = gens[0]
            pdev = g0.device if g0 is not None else device
            for i in range(L, num_frames, s):
                start = max(0, i - L)
                n = min(num_frames, start + s) - start
                if n == 0:
                    break
                idx = (start + torch.randperm(n, generator=g0, device=pdev)).to(latents.device)
                end = min(num_frames, i + n)
                latents[:, :, i:end] = latents[:, :, idx[:end - i]]
        return latents

    # ------------------------------------------------------------------ FreeInit
    def enable_free_init(self, num_iters=3, use_fast_sampling=False, method="butterworth", order=4,
                         spatial_stop_frequency=0.25, temporal_stop_frequency=0.25):
        """diffusers' FreeInitMixin.enable_free_init: __call__ samples the video num_iters times;
        between two runs the finished latents are noised back to the last training timestep with
        the initial noise and their high spatio-temporal frequencies replaced by fresh noise
        through a 3-D low-pass over (frames, height, width) (ops.free_init_filter).
        use_fast_sampling runs iteration i over max(1, int(steps / num_iters * (i + 1))) steps."""
        if int(num_iters) != num_iters or num_iters < 1:
            raise ValueError(f"num_iters must be an integer >= 1, got {num_iters!r}")
        if method not in ops.FREE_INIT_METHODS:
            raise NotImplementedError("`filter_type` must be one of gaussian, butterworth or ideal")
        if int(order) != order or order < 1:
            raise ValueError(f"order must be an integer >= 1, got {order!r}")
        if spatial_stop_frequency < 0 or temporal_stop_frequency < 0:
            raise ValueError(f"stop frequencies must be >= 0, got spatial_stop_frequency={spatial_stop_frequency}, "
                             f"temporal_stop_frequency={temporal_stop_frequency}")
        self._free_init_num_iters = int(num_iters)
        self._free_init_use_fast_sampling = bool(use_fast_sampling)
        self._free_init_method = method
        self._free_init_order = int(order)
        self._free_init_spatial_stop_frequency = spatial_stop_frequency
        self._free_init_temporal_stop_frequency = temporal_stop_frequency

    def disable_free_init(self):
        self._free_init_num_iters = None

    @property
    def free_init_enabled(self) -> bool:
        return getattr(self, "_free_init_num_iters", None) is not None

    def _free_init_steps(self, num_inference_steps, iteration):
        """The step count of one FreeInit iteration."""
        if self._free_init_use_fast_sampling:
            return max(1, int(num_inference_steps / self._free_init_num_iters * (iteration + 1)))
        return num_inference_steps

    def _apply_free_init(self, latents, iteration, num_inference_steps, generator=None):
        """diffusers' FreeInitMixin._apply_free_init -> (latents, timesteps).  Iteration 0 keeps a
        clone of the latents as the initial noise (and builds the call's filter table and
        scratch); a later one returns
          free_init_filter(add_noise(latents, initial_noise, num_train_timesteps - 1), z_rand),
        z_rand one fp32 randn_tensor draw from `generator`.  Then scheduler.set_timesteps with the
        iteration's step count."""
        if iteration == 0:
            F, H, W = latents.shape[-3:]
            self._free_init_initial_noise = latents.detach().clone()
            self._free_init_table = ops.free_init_table(
                F, H, W, self._free_init_method, self._free_init_order, self._free_init_spatial_stop_frequency,
                self._free_init_temporal_stop_frequency, device=latents.device)
            self._free_init_scratch = torch.empty(latents.numel() // W * 2 * (W // 2 + 1), device=latents.device,
                                                  dtype=torch.float32)
        else:
            t = self.scheduler.config.num_train_timesteps - 1
            z_t = self.scheduler.add_noise(latents, self._free_init_initial_noise,
                                           torch.full((latents.shape[0],), t)).to(torch.float32).contiguous()
            z_rand = randn_tensor(latents.shape, generator=generator, device=latents.device, dtype=torch.float32)
            latents = ops.free_init_filter(z_t, z_rand.contiguous(), self._free_init_table,
                                           scratch=self._free_init_scratch)
        self.scheduler.set_timesteps(self._free_init_steps(num_inference_steps, iteration))
        return latents, self.scheduler.timesteps

    # ------------------------------------------------------------------ the scheduler's step noise
    @property
    def _lcm(self) -> bool:
        return getattr(self.scheduler, "kind", None) == "lcm"

    @property
    def _dpm(self) -> bool:
        return getattr(self.scheduler, "kind", None) == "dpm"

    @property
    def _unipc(self) -> bool:
        return getattr(self.scheduler, "kind", None) == "unipc"

    @property
    def _dpm_sde(self) -> bool:
        return self._dpm and self.scheduler.sde

    @property
    def _euler_a(self) -> bool:
        return getattr(self.scheduler, "kind", None) == "euler_a"

    def _refuse_scheduler_combinations(self):
        """What a stochastic or multistep scheduler does not combine with."""
        if self._lcm and self.dist is not None:
            raise NotImplementedError("LCMScheduler with a frame-sharded pipeline (dist=) is not supported: the "
                                      "per-step noise slabs are not sharded over the ranks' frames")
        if self._dpm_sde and self.dist is not None:
            raise NotImplementedError("DPMSolverMultistepScheduler's algorithm_type 'sde-dpmsolver++' with a "
                                      "frame-sharded pipeline (dist=) is not supported: the per-step noise slabs are "
                                      "not sharded over the ranks' frames ('dpmsolver++' is)")
        if self._euler_a and self.dist is not None:
            raise NotImplementedError("EulerAncestralDiscreteScheduler with a frame-sharded pipeline (dist=) is not "
                                      "supported: the per-step noise slabs are not sharded over the ranks' frames")
        if self._dpm and self.free_init_enabled:
            raise NotImplementedError("FreeInit with DPMSolverMultistepScheduler is not supported: diffusers' "
                                      "add_noise at a timestep outside the schedule falls back to the last sigma; "
                                      "disable_free_init(), or use DDIMScheduler")
        if self._unipc and self.free_init_enabled:
            raise NotImplementedError("FreeInit with UniPCMultistepScheduler is not supported: diffusers' "
                                      "add_noise at a timestep outside the schedule falls back to the last sigma; "
                                      "disable_free_init(), or use DDIMScheduler")

    def _step_noise(self, latents, n_steps, generator, draw=True):
        """The scheduler's step noise, None for a deterministic one.
        LCM: its n_steps - 1 stochastic steps', [n_steps - 1, *latents.shape]: one randn_tensor of
        the latents' shape per non-final step, in step order, on the call's generator and in the
        dtype the initial noise is drawn in (diffusers draws in model_output.dtype, the pipeline's
        torch_dtype).  The SDE type of DPMSolverMultistepScheduler: [n_steps, *latents.shape], one
        fp32 draw per step, the last included (diffusers draws there too, and multiplies by 0).
        EulerAncestralDiscreteScheduler: [n_steps, *latents.shape], one draw per step in the pipeline's
        torch_dtype as for LCM, the last included (diffusers draws there too; its sigma_up is 0).
        Either way that is the draw order of diffusers' loop, where scheduler.step is the only
        thing that draws.  draw=False gives zeros of that shape (a loop built before its noise is
        known)."""
        if self._dpm_sde:
            if not draw:
                return torch.zeros((n_steps,) + tuple(latents.shape), device=latents.device, dtype=torch.float32)
            return torch.stack([randn_tensor(latents.shape, generator=generator, device=latents.device,
                                             dtype=torch.float32) for _ in range(n_steps)])
        if self._euler_a:
            if not draw:
                return torch.zeros((n_steps,) + tuple(latents.shape), device=latents.device, dtype=torch.float32)
            dtype = self.torch_dtype or torch.float32
            return torch.stack([randn_tensor(latents.shape, generator=generator, device=latents.device, dtype=dtype)
                                for _ in range(n_steps)]).to(torch.float32)
        if not self._lcm:
            return None
        shape = (max(n_steps - 1, 0),) + tuple(latents.shape)
        if not draw or n_steps <= 1:
            return torch.zeros(shape, device=latents.device, dtype=torch.float32)
        dtype = self.torch_dtype or torch.float32
        return torch.stack([randn_tensor(latents.shape, generator=generator, device=latents.device, dtype=dtype)
                            for _ in range(n_steps - 1)]).to(torch.float32)

    def _free_init_sample(self, latents, num_inference_steps, generator, make_loop, schedule=lambda ts: ts):
        """The FreeInit iterations around one DenoiseLoop: make_loop(timesteps) builds it, once, for
        the longest schedule; schedule(timesteps) is what an iteration runs of its timesteps (the
        video-to-video pipeline's cut by strength).  -> the last iteration's latents."""
        n = self._free_init_num_iters
        self.scheduler.set_timesteps(max(self._free_init_steps(num_inference_steps, i) for i in range(n)))
        now = schedule(self.scheduler.timesteps)
        loop = make_loop(now).prime()
        try:
            for i in range(n):
                latents, ts = self._apply_free_init(latents, i, num_inference_steps, generator)
                ts = schedule(ts)
                if len(ts) != len(now) or not torch.equal(torch.as_tensor(ts).cpu(), torch.as_tensor(now).cpu()):
                    loop.reschedule(ts)
                    now = ts
                # an LCM schedule: this iteration's step noise, drawn after _apply_free_init's draws
                loop.reset(latents, step_noise=self._step_noise(latents, len(ts), generator))
                latents = loop.run()
        finally:
            self._free_init_initial_noise = self._free_init_table = self._free_init_scratch = None
        return latents

    # ------------------------------------------------------------------ IP-Adapter
    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder=None,
                        weight_name=None, image_encoder_folder="image_encoder", **unused):
        """diffusers' load_ip_adapter over LOCAL files (vdiff.pretrained.read_ip_adapter): the plain
        adapter's image_proj.* become self.image_projection, its ip_adapter.{id}.to_k_ip / to_v_ip
        weights go to the UNet's spatial cross-attentions (ids 1, 3, 5, ... in
        pretrained.IP_ADAPTER_BLOCK_ORDER).  image_encoder_folder (relative to subfolder when it
        has no "/", as diffusers) is loaded as a vdiff.CLIPVisionModelWithProjection when the
        pipeline has no image encoder yet and the folder exists; without one only
        ip_adapter_image_embeds= can be used.  The scale starts at 1.0."""
        from . import pretrained as P
        from .image_processor import CLIPImageProcessor
        from .models.clip import ImageProjection
        src = pretrained_model_name_or_path_or_dict
        image_proj, ip = P.read_ip_adapter(src, subfolder, weight_name or P.IP_ADAPTER_WEIGHT_NAME)
        P.check_ip_adapter_variant(image_proj, ip)
        unet = self.unet
        cross = unet.config["cross_attention_dim"]
        kv = P.ip_adapter_kv_weights(ip, len(unet.spatial_cross_attentions()))
        proj = ImageProjection.from_state_dict(image_proj, cross)
        if not 1 <= proj.num_image_text_embeds <= 64:
            raise NotImplementedError(f"{proj.num_image_text_embeds} image tokens: the attention tail holds 1..64")
        unet.unload_ip_adapter()  # a second load replaces the first; an image encoder already set is kept
        unet.set_ip_adapter_weights(kv, scale=1.0)
        self.image_projection = proj.to(device=unet.device, dtype=torch.bfloat16)
        if unet.device.type == "cuda":
            self.image_projection.prepare()
        if self.image_encoder is None and image_encoder_folder is not None and not isinstance(src, dict):
            root = P._local_dir(src, "load_ip_adapter")
            rel = Path(image_encoder_folder)
            folder = root / rel if "/" in str(image_encoder_folder) or not subfolder else root / subfolder / rel
            if folder.is_dir():
                self.image_encoder = P.load_image_encoder(folder, device=unet.device)
        if self.feature_extractor is None:
            size = 224 if self.image_encoder is None else self.image_encoder.config["image_size"]
            self.feature_extractor = CLIPImageProcessor(size=size, crop_size=size)
        return self

    def unload_ip_adapter(self):
        """Back to the text-only pipeline: the UNet's parameters, state_dict keys, prepared operands
        and launches are those of a model that never loaded an adapter."""
        self.unet.unload_ip_adapter()
        self.image_projection = None
        self.image_encoder = None
        self.feature_extractor = None

    def set_ip_adapter_scale(self, scale):
        if self.image_projection is None:
            raise ValueError("set_ip_adapter_scale: no IP-Adapter loaded")
        self.unet.set_ip_adapter_scale(scale)

    def encode_image(self, image):
        """(image_embeds, zeros_like(image_embeds)) as diffusers' encode_image without hidden states:
        bf16 (B, clip_dim) from the CLIP vision tower."""
        if self.image_encoder is None:
            raise ValueError("ip_adapter_image needs an image encoder: load_ip_adapter(..., image_encoder_folder=...) "
                             "or pipe.image_encoder = vdiff.CLIPVisionModelWithProjection(...)")
        if not isinstance(image, torch.Tensor) or image.dim() != 4:
            image = self.feature_extractor(image, return_tensors="pt").pixel_values
        e = self.image_encoder(image.to(self.image_encoder.device, torch.bfloat16)).image_embeds
        return e, torch.zeros_like(e)

    def prepare_ip_adapter_image_embeds(self, ip_adapter_image, ip_adapter_image_embeds, n_prompts,
                                        num_videos_per_prompt, do_cfg):
        """The projected image tokens [Bt, n, cross_attention_dim] for DenoiseLoop (uncond half
        first under CFG), or None when neither argument is given.  diffusers' order: image_embeds
        from the encoder, the negative zeros_like, [negative; positive] under CFG, each
        repeat_interleave'd by num_videos_per_prompt, then the projection.  Precomputed embeds are
        (B, 1, clip_dim), or (2B, 1, clip_dim) with the negative half first under CFG.  One image
        for several prompts is shared by all of them."""
        if ip_adapter_image is None and ip_adapter_image_embeds is None:
            return None
        if self.image_projection is None:
            raise ValueError("ip_adapter_image / ip_adapter_image_embeds given, but no IP-Adapter is loaded "
                             "(pipe.load_ip_adapter(...))")
        if ip_adapter_image is not None and ip_adapter_image_embeds is not None:
            raise ValueError("pass ip_adapter_image or ip_adapter_image_embeds, not both")
        dev = self.unet.device
        if ip_adapter_image_embeds is not None:
            e = ip_adapter_image_embeds
            if isinstance(e, (list, tuple)):
                if len(e) != 1:
                    raise NotImplementedError("a list of IP-Adapters (multiple image prompts) is not supported")
                e = e[0]
            e = e.to(dev, torch.bfloat16)
            e = e.reshape(e.shape[0], -1)
            neg, pos = e.chunk(2) if do_cfg else (None, e)
        else:
            pos, neg = self.encode_image(ip_adapter_image)
            if not do_cfg:
                neg = None
        if pos.shape[0] == 1 and n_prompts > 1:
            pos = pos.expand(n_prompts, -1)
            neg = None if neg is None else neg.expand(n_prompts, -1)
        if pos.shape[0] != n_prompts:
            raise ValueError(f"{pos.shape[0]} image prompts for {n_prompts} prompts")
        pos = pos.repeat_interleave(num_videos_per_prompt, 0)
        if neg is not None:
            pos = torch.cat([neg.repeat_interleave(num_videos_per_prompt, 0), pos])
        return self.image_projection(pos.contiguous())

    def encode_prompt(self, prompt, batch, clip_skip=None):
        """(batch, 77, dim) embeddings of a prompt or a list of prompts.  With a tokenizer and a
        CLIPTextModel: the whole list is tokenized (padding="max_length", truncation) and encoded
        in ONE batched forward; clip_skip as diffusers, final_layer_norm(hidden_states[-(clip_skip
        + 1)]).  Without a tokenizer the stub encoder is called per prompt."""
        if isinstance(prompt, str):
            prompt = [prompt] * batch
        if self.tokenizer is None:
            if clip_skip is not None:
                raise ValueError("clip_skip needs a CLIPTextModel and a tokenizer")
            return torch.stack([self.text_encoder(p) for p in prompt])
        enc = self.text_encoder
        ids = self.tokenizer(list(prompt), padding="max_length", max_length=self.tokenizer.model_max_length,
                             truncation=True, return_tensors="pt").input_ids.to(enc.device)
        if clip_skip is None:
            return enc(ids)[0]
        hs = enc(ids, output_hidden_states=True).hidden_states
        return enc.text_model.final_layer_norm(hs[-(clip_skip + 1)])

    @staticmethod
    def _prompt_travel_keys(prompt, num_frames, name="prompt"):
        """diffusers' _encode_prompt_free_noise normalisation of one side: a str is {0: str}; int
        keys, str values; sorted by frame; the first key 0, the last <= num_frames - 1, where the
        last prompt is repeated when no key names it -> (frame indices, texts)."""
        if isinstance(prompt, str):
            prompt = {0: prompt}
        if not isinstance(prompt, dict):
            raise ValueError(f"Expected `{name}` to be either `str` or `dict`, got {type(prompt).__name__}.")
        if not prompt or not all(isinstance(k, int) and not isinstance(k, bool) for k in prompt) or \
                not all(isinstance(v, str) for v in prompt.values()):
            raise ValueError(f"Expected integer keys and string values for `{name}` dict.")
        frames = sorted(prompt)
        if frames[0] != 0:
            raise ValueError(f"The minimum frame index in `{name}` dict must be 0 or missing.")
        if frames[-1] >= num_frames:
            raise ValueError(f"The maximum frame index in `{name}` dict must be lesser than `num_frames` and follow "
                             "0-based indexing.")
        texts = [prompt[f] for f in frames]
        if frames[-1] != num_frames - 1:
            frames, texts = frames + [num_frames - 1], texts + [texts[-1]]
        return frames, texts

    def encode_prompt_free_noise(self, prompt, negative_prompt, num_frames, num_videos_per_prompt=1,
                                 do_classifier_free_guidance=True, clip_skip=None):
        """diffusers' AnimateDiffFreeNoiseMixin._encode_prompt_free_noise with its default linear
        interpolation (FreeNoise prompt travel): `prompt` is a str or a {frame: text} dict, and so
        is `negative_prompt`, with keys of its own.  Every key prompt of both sides goes through
        the text encoder in ONE batched forward; each side's [K, 77, dim] key embeddings are
        interpolated frame by frame by one launch (ops.prompt_lerp, vd_rows_eltwise op 9).
        -> (prompt_embeds, negative_prompt_embeds or None), each bf16 [num_videos_per_prompt,
        num_frames, 77, dim] on the UNet's device: the per-frame form __call__ takes as prompt_embeds /
        negative_prompt_embeds; flattened over (video, frame) it is DenoiseLoop's per-frame form."""
        pf, pt = self._prompt_travel_keys(prompt, num_frames)
        nf, nt = [], []
        if do_classifier_free_guidance:
            nf, nt = self._prompt_travel_keys("" if negative_prompt is None else negative_prompt, num_frames,
                                              "negative_prompt")
        keys = self.encode_prompt(nt + pt, len(nt) + len(pt), clip_skip=clip_skip)
        keys = keys.to(self.unet.device, torch.bfloat16).contiguous()
        L, D = keys.shape[1], keys.shape[2]

        def travel(k, frames):
            rows = ops.prompt_lerp(k.reshape(len(frames) * L, D), frames, 1, num_frames, L)
            return rows.view(1, num_frames, L, D).repeat(num_videos_per_prompt, 1, 1, 1)

        pos = travel(keys[len(nt):], pf)
        return pos, (travel(keys[:len(nt)], nf) if do_classifier_free_guidance else None)

    @staticmethod
    def _is_per_frame(e):
        """Precomputed embeddings in the per-frame form are 4-D, [videos, F, tokens, dim]; 3-D ones
        are per video, [videos, tokens, dim], as they always were."""
        return e is not None and e.dim() == 4

    def _refuse_prompt_dict(self, prompt, negative_prompt):
        """A {frame: text} dict needs FreeNoise; refused before any tokenizer or device work."""
        if (isinstance(prompt, dict) or isinstance(negative_prompt, dict)) and not self.free_noise_enabled:
            raise NotImplementedError("a {frame: text} prompt dict (FreeNoise prompt travel) needs FreeNoise: call "
                                      "enable_free_noise() first")

    def _prompt_travel_ehs(self, prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, num_frames, do_cfg,
                           num_videos_per_prompt, clip_skip, ip_given, unused):
        """The per-frame text of a prompt-travel call -> (ehs [Bt * F, L, D] with the unconditional
        half first under CFG, B), or None for a call in today's per-video form.  A call is a
        prompt-travel call when a prompt is a dict or precomputed embeddings are per frame."""
        travel = isinstance(prompt, dict) or isinstance(negative_prompt, dict)
        pre = self._is_per_frame(prompt_embeds) or self._is_per_frame(negative_prompt_embeds)
        if not travel and not pre:
            return None
        if not self.free_noise_enabled:
            raise NotImplementedError("per-frame prompt embeddings (FreeNoise prompt travel) need FreeNoise: call "
                                      "enable_free_noise() first")
        if ip_given:
            raise NotImplementedError("FreeNoise prompt travel together with an IP-Adapter image prompt is not "
                                      "supported: the text + image K/V rows are laid out per video")
        if unused.get("cfg_shard") is not None:
            raise NotImplementedError("FreeNoise prompt travel together with cfg_shard is not supported")
        if self.dist is not None:
            raise NotImplementedError("FreeNoise prompt travel with a frame-sharded pipeline (dist=) is not supported")
        pos, neg = prompt_embeds, negative_prompt_embeds
        if pos is None or (do_cfg and neg is None):
            if pos is None and prompt is None:
                raise ValueError("prompt or prompt_embeds required")
            if isinstance(prompt, (list, tuple)) or isinstance(negative_prompt, (list, tuple)):
                raise ValueError("Expected `prompt` and `negative_prompt` to be either `str` or `dict` in a "
                                 "prompt-travel call (one travel per call, as diffusers).")
            p, n = self.encode_prompt_free_noise(prompt if pos is None else "", negative_prompt, num_frames,
                                                 num_videos_per_prompt, do_cfg and neg is None, clip_skip)
            pos = p if pos is None else pos
            neg = n if neg is None else neg
        dev = self.unet.device

        def form(e, what, repeat):
            e = e.to(dev, torch.bfloat16)
            if not self._is_per_frame(e):  # per-video beside a per-frame side: every frame reads the same text
                e = e[:, None].expand(-1, num_frames, -1, -1)
            if e.shape[1] != num_frames:
                raise ValueError(f"{what} of shape {tuple(e.shape)}: the per-frame form is [videos, {num_frames}, "
                                 "tokens, dim]")
            return e.repeat_interleave(num_videos_per_prompt, 0) if repeat else e

        pos = form(pos, "prompt_embeds", prompt_embeds is not None)
        B = pos.shape[0]
        if do_cfg:
            neg = form(neg, "negative_prompt_embeds", negative_prompt_embeds is not None)
            if neg.shape != pos.shape:
                raise ValueError(f"negative embeddings of shape {tuple(neg.shape)} for positive {tuple(pos.shape)}")
            pos = torch.cat([neg, pos])
        return pos.reshape(-1, pos.shape[2], pos.shape[3]).contiguous(), B

    @torch.no_grad()
    def decode_latents(self, latents):
        """diffusers AnimateDiffPipeline.decode_latents: latents / scaling_factor, frames
        batched frame-major through vae.decode, -> (B, 3, F, H, W) fp32 in about [-1, 1]."""
        if self.vae is None:
            raise ValueError("this pipeline has no VAE (pass vae=vdiff.AutoencoderKL(...).to(...))")
        B, Cc, Fr, h, w = latents.shape
        z = latents.float() / self.vae.config["scaling_factor"]
        z = z.permute(0, 2, 1, 3, 4).reshape(B * Fr, Cc, h, w)
        img = self.vae.decode(z).sample
        return img[None].reshape((B, Fr) + tuple(img.shape[1:])).permute(0, 2, 1, 3, 4).float()

    @staticmethod
    def postprocess_video(video, output_type):
        """diffusers VideoProcessor.postprocess_video for "pt" / "np" / "pil": per video, frames
        first, denormalised (x / 2 + 0.5).clamp(0, 1); "pil" -> a list (per video) of lists of
        PIL images."""
        v = (video / 2 + 0.5).clamp(0, 1).permute(0, 2, 1, 3, 4)      # (B, F, 3, H, W)
        if output_type == "pt":
            return v
        arr = v.permute(0, 1, 3, 4, 2).float().cpu().numpy()           # (B, F, H, W, 3)
        if output_type == "np":
            return arr
        return [numpy_to_pil(a) for a in arr]

    def _make_loop(self, *args, **kwargs):
        """The call's DenoiseLoop (a subclass adds what its loop needs, e.g. control=)."""
        return DenoiseLoop(*args, **kwargs)

    def prepare_latents(self, batch, num_frames, h, w, generator=None, latents=None):
        """diffusers AnimateDiffPipeline.prepare_latents -> fp32 on the GPU, x init_noise_sigma.
        The draw follows randn_tensor: on the generator's device (a CPU generator from 05:156's
        torch.manual_seed, a CUDA one from 01:103's torch.Generator("cuda")), in the pipeline's
        torch_dtype (float16 in the reference, 01:21 / 05:35; fp32 when the pipeline was loaded
        with torch_dtype=None, as diffusers draws in prompt_embeds.dtype), then moved."""
        if self.free_noise_enabled:
            latents = self._prepare_latents_free_noise(batch, num_frames, h, w, generator=generator, latents=latents)
        elif latents is None:
            shape = (batch, self.unet.config["in_channels"], num_frames, h, w)
            dtype = self.torch_dtype or torch.float32
            latents = randn_tensor(shape, generator=generator, device=self.unet.device, dtype=dtype)
        return latents.to(self.unet.device, torch.float32) * self.scheduler.init_noise_sigma

    @torch.no_grad()
    def __call__(self, prompt=None, num_frames=16, height=None, width=None, num_inference_steps=50,
                 guidance_scale=7.5, negative_prompt=None, num_videos_per_prompt=1, eta=0.0,
                 generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                 output_type="pil", return_dict=True, use_graph=True, clip_skip=None,
                 ip_adapter_image=None, ip_adapter_image_embeds=None, **unused):
        if eta != 0.0:
            raise NotImplementedError("eta > 0")
        if self.free_init_enabled and self.dist is not None:
            raise NotImplementedError("FreeInit with a frame-sharded pipeline (dist=) is not supported: the filter "
                                      "needs every frame of a video and the ranks would have to agree on z_rand")
        self._refuse_scheduler_combinations()
        self._refuse_prompt_dict(prompt, negative_prompt)
        if output_type not in ("latent", "pt", "np", "pil"):
            raise NotImplementedError(f"output_type {output_type!r}: use 'pil', 'pt', 'np' or 'latent'")
        if output_type != "latent" and self.vae is None:
            raise ValueError(f"output_type {output_type!r} needs a VAE: AnimateDiffPipeline(..., vae=...)")
        dev = self.unet.device
        sample = self.unet.config["sample_size"]
        h = (height or sample * 8) // 8
        w = (width or sample * 8) // 8
        do_cfg = guidance_scale > 1
        # FreeNoise prompt travel: per-frame text, [Bt * F, L, D] for the loop
        travel = self._prompt_travel_ehs(prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, num_frames,
                                         do_cfg, num_videos_per_prompt, clip_skip,
                                         ip_adapter_image is not None or ip_adapter_image_embeds is not None, unused)
        if travel is None and prompt_embeds is None:
            if prompt is None:
                raise ValueError("prompt or prompt_embeds required")
            pos = [prompt] if isinstance(prompt, str) else list(prompt)
            n = len(pos)
            if self.tokenizer is not None and do_cfg and negative_prompt_embeds is None:
                # the positive and the negative prompts in one encoder forward
                neg = negative_prompt if negative_prompt is not None else ""
                neg = [neg] * n if isinstance(neg, str) else list(neg)
                if len(neg) != n:
                    raise ValueError(f"{len(neg)} negative prompts for {n} prompts")
                both = self.encode_prompt(neg + pos, 2 * n, clip_skip=clip_skip)
                negative_prompt_embeds = both[:n].repeat_interleave(num_videos_per_prompt, 0)
                prompt_embeds = both[n:]
            else:
                prompt_embeds = self.encode_prompt(pos, n, clip_skip=clip_skip)
        if travel is not None:
            ehs, B = travel
        else:
            B = prompt_embeds.shape[0] * num_videos_per_prompt
            prompt_embeds = prompt_embeds.repeat_interleave(num_videos_per_prompt, 0)
            if do_cfg:
                if negative_prompt_embeds is None:
                    negative_prompt_embeds = self.encode_prompt(negative_prompt or "", B, clip_skip=clip_skip)
                ehs = torch.cat([negative_prompt_embeds.to(prompt_embeds), prompt_embeds])
            else:
                ehs = prompt_embeds
        ip_embeds = self.prepare_ip_adapter_image_embeds(ip_adapter_image, ip_adapter_image_embeds,
                                                         B // num_videos_per_prompt, num_videos_per_prompt, do_cfg)
        self.scheduler.set_timesteps(num_inference_steps)
        latents = self.prepare_latents(B, num_frames, h, w, generator=generator, latents=latents)
        local = latents
        if self.dist is not None:
            fl = self.dist.frames_local(num_frames)
            local = latents[:, :, self.dist.rank * fl:(self.dist.rank + 1) * fl]
        if self.free_init_enabled:
            out = self._free_init_sample(
                latents, num_inference_steps, generator,
                lambda ts: self._make_loop(self.unet, self.scheduler, latents, ehs, guidance_scale, timesteps=ts,
                                           use_graph=use_graph, ip_embeds=ip_embeds,
                                           step_noise=self._step_noise(latents, len(ts), None, draw=False)))
        else:
            # an LCM schedule's step noise: drawn right after the initial latents, in step order
            step_noise = self._step_noise(latents, len(self.scheduler.timesteps), generator)
            loop = self._make_loop(self.unet, self.scheduler, local, ehs, guidance_scale,
                                   use_graph=use_graph, ip_embeds=ip_embeds, step_noise=step_noise).prime()
            out = loop.run()
        if self.dist is not None:
            out = self.dist.all_gather_frames(out)
        if output_type != "latent":
            out = self.postprocess_video(self.decode_latents(out), output_type)
        return AnimateDiffPipelineOutput(frames=out) if return_dict else (out,)


def preprocess_video(video, height=None, width=None):
    """The video-to-video input -> (B, 3, F, H, W) fp32 in [-1, 1] on the CPU.  Accepted: a list of
    PIL frames or a list of such lists; an ndarray (F, H, W, 3) or (B, F, H, W, 3) in [0, 1]; a
    tensor (F, 3, H, W) or (B, F, 3, H, W) in [0, 1].  height / width default to the video's own
    size.  PIL frames of another size are resized (LANCZOS); arrays and tensors are refused."""
    return (2.0 * decode_video_frames(video, height, width) - 1.0).permute(0, 2, 1, 3, 4).contiguous()


def decode_video_frames(video, height=None, width=None):
    """preprocess_video's decoding, left in [0, 1]: -> (B, F, 3, H, W) fp32 on the CPU."""
    import numpy as np
    if isinstance(video, (list, tuple)) and len(video) > 0 and not torch.is_tensor(video[0]) \
            and not isinstance(video[0], np.ndarray):
        from PIL import Image
        vids = [list(video)] if isinstance(video[0], Image.Image) else [list(v) for v in video]
        if not all(len(v) > 0 and all(isinstance(f, Image.Image) for f in v) for v in vids):
            raise ValueError("video: a list of PIL frames, or a list of such lists")
        if len({len(v) for v in vids}) != 1:
            raise ValueError("video: every video of the batch needs the same number of frames")
        w0, h0 = vids[0][0].size
        height, width = height or h0, width or w0
        arr = np.stack([np.stack([np.asarray((f if f.size == (width, height)
                                              else f.resize((width, height), Image.LANCZOS)).convert("RGB"),
                                             dtype=np.float32) / 255.0 for f in v]) for v in vids])
        x = torch.from_numpy(arr).permute(0, 1, 4, 2, 3)              # (B, F, 3, H, W)
    elif isinstance(video, np.ndarray):
        if video.ndim not in (4, 5) or video.shape[-1] != 3:
            raise ValueError(f"video array: (F, H, W, 3) or (B, F, H, W, 3), got {video.shape}")
        x = torch.from_numpy(np.ascontiguousarray(video)).float()
        x = (x[None] if x.dim() == 4 else x).permute(0, 1, 4, 2, 3)
    elif torch.is_tensor(video):
        if video.dim() not in (4, 5) or video.shape[-3] != 3:
            raise ValueError(f"video tensor: (F, 3, H, W) or (B, F, 3, H, W), got {tuple(video.shape)}")
        x = video.detach().float().cpu()
        x = x[None] if x.dim() == 4 else x
    else:
        raise ValueError("video: PIL frames, an ndarray or a tensor")
    H, W = x.shape[-2:]
    if (height or H) != H or (width or W) != W:
        raise ValueError(f"video is {H} x {W}, asked for {height} x {width}: only PIL frames are resized")
    if H % 8 or W % 8:
        raise ValueError(f"video height and width must be multiples of 8, got {H} x {W}")
    return x


class AnimateDiffVideoToVideoPipeline(AnimateDiffPipeline):
    """diffusers AnimateDiffVideoToVideoPipeline: `pipe(video=, prompt=, strength=, ...)` encodes
    the video, noises it to the timestep `strength` picks and runs the text-to-video pipeline's
    denoising loop (the same captured graph) over the remaining timesteps.  Parity to diffusers
    is unpinned, as the decoder's."""

    vae_encoder = True

    def __init__(self, unet, scheduler=None, text_encoder=None, vae=None, dist=None, tokenizer=None):
        super().__init__(unet, scheduler, text_encoder=text_encoder, vae=vae, dist=dist, tokenizer=tokenizer)
        if vae is None or getattr(vae, "encoder", None) is None:
            raise ValueError("AnimateDiffVideoToVideoPipeline needs a VAE with its encoder: "
                             "AutoencoderKL(config, encoder=True), or a vae/ checkpoint that holds every "
                             "encoder.* and quant_conv.* tensor")

    def get_timesteps(self, num_inference_steps, strength):
        """diffusers get_timesteps: the last min(int(n * strength), n) timesteps of the schedule
        (set_timesteps first) and their count."""
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"strength must be in (0, 1], got {strength}")
        init = min(int(num_inference_steps * strength), num_inference_steps)
        if init == 0:
            raise ValueError(f"strength {strength} with {num_inference_steps} steps leaves no step to run")
        t_start = max(num_inference_steps - init, 0)
        ts = self.scheduler.timesteps[t_start * self.scheduler.order:]
        return ts, num_inference_steps - t_start

    @torch.no_grad()
    def encode_video(self, video, generator=None):
        """One video (F, 3, H, W) in [-1, 1] -> (F, C, h, w) latents x scaling_factor: chunks of
        vae.frames_per_chunk frames, each chunk's posterior sampled with `generator` in turn."""
        n = self.vae.frames_per_chunk
        lat = [self.vae.encode(video[i:i + n]).latent_dist.sample(generator=generator)
               for i in range(0, video.shape[0], n)]
        return self.vae.config["scaling_factor"] * torch.cat(lat)

    @torch.no_grad()
    def prepare_latents(self, video, timestep, generator=None, latents=None):
        """diffusers AnimateDiffVideoToVideoPipeline.prepare_latents -> (B, C, F, h, w) fp32 on the
        GPU.  video (B, 3, F, H, W) in [-1, 1]; `latents` given bypasses encoding and noising.
        Draw order on `generator` (one stream, as diffusers):
          1. per video, per chunk of vae.frames_per_chunk frames in order: the posterior's
             randn (chunk frames, C, h, w), drawn in fp32 (the moments' dtype here);
          2. the latents x scaling_factor, stacked to (B, F, C, h, w);
          3. ONE noise tensor (B, F, C, h, w) in the pipeline's torch_dtype (fp32 when None);
          4. scheduler.add_noise(latents, noise, timestep);
          5. permute to (B, C, F, h, w)."""
        dev = self.unet.device
        if latents is not None:
            return latents.to(dev, torch.float32)
        frames = video.permute(0, 2, 1, 3, 4)                             # (B, F, 3, H, W)
        init = torch.stack([self.encode_video(v, generator) for v in frames]).to(dev, torch.float32)
        noise = randn_tensor(init.shape, generator=generator, device=dev, dtype=self.torch_dtype or torch.float32)
        x = self.scheduler.add_noise(init, noise.float(), torch.as_tensor(timestep).reshape(-1)[:1])
        return x.permute(0, 2, 1, 3, 4).contiguous()

    @torch.no_grad()
    def __call__(self, video=None, prompt=None, negative_prompt=None, height=None, width=None,
                 num_inference_steps=50, guidance_scale=7.5, strength=0.8, num_videos_per_prompt=1, eta=0.0,
                 generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                 output_type="pil", return_dict=True, clip_skip=None, use_graph=True,
                 ip_adapter_image=None, ip_adapter_image_embeds=None, **unused):
        if eta != 0.0:
            raise NotImplementedError("eta > 0")
        if self.free_init_enabled and self.dist is not None:
            raise NotImplementedError("FreeInit with a frame-sharded pipeline (dist=) is not supported: the filter "
                                      "needs every frame of a video and the ranks would have to agree on z_rand")
        if output_type not in ("latent", "pt", "np", "pil"):
            raise NotImplementedError(f"output_type {output_type!r}: use 'pil', 'pt', 'np' or 'latent'")
        if video is None and latents is None:
            raise ValueError("video or latents required")
        self._refuse_scheduler_combinations()
        self._refuse_prompt_dict(prompt, negative_prompt)
        do_cfg = guidance_scale > 1
        # FreeNoise prompt travel: per-frame text over the frames the video (or the latents) has
        travel = None
        if isinstance(prompt, dict) or isinstance(negative_prompt, dict) or self._is_per_frame(prompt_embeds) or \
                self._is_per_frame(negative_prompt_embeds):
            if latents is None:  # the frame count comes from the video: preprocessed here, once
                video = preprocess_video(video, height, width)
            nf = latents.shape[2] if latents is not None else video.shape[2]
            travel = self._prompt_travel_ehs(prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, nf,
                                             do_cfg, num_videos_per_prompt, clip_skip,
                                             ip_adapter_image is not None or ip_adapter_image_embeds is not None,
                                             unused)
        if travel is not None:
            ehs, B = travel
        else:
            if prompt_embeds is None:
                if prompt is None:
                    raise ValueError("prompt or prompt_embeds required")
                pos = [prompt] if isinstance(prompt, str) else list(prompt)
                prompt_embeds = self.encode_prompt(pos, len(pos), clip_skip=clip_skip)
            B = prompt_embeds.shape[0] * num_videos_per_prompt
            prompt_embeds = prompt_embeds.repeat_interleave(num_videos_per_prompt, 0)
            if do_cfg:
                if negative_prompt_embeds is None:
                    negative_prompt_embeds = self.encode_prompt(negative_prompt or "", B, clip_skip=clip_skip)
                ehs = torch.cat([negative_prompt_embeds.to(prompt_embeds), prompt_embeds])
            else:
                ehs = prompt_embeds
        ip_embeds = self.prepare_ip_adapter_image_embeds(ip_adapter_image, ip_adapter_image_embeds,
                                                         B // num_videos_per_prompt, num_videos_per_prompt, do_cfg)
        self.scheduler.set_timesteps(num_inference_steps)
        ts, _ = self.get_timesteps(num_inference_steps, strength)
        if latents is None:
            if travel is None:
                video = preprocess_video(video, height, width)
            if video.shape[0] == 1 and B > 1:
                video = video.expand(B, -1, -1, -1, -1)
            if video.shape[0] != B:
                raise ValueError(f"{video.shape[0]} videos for a batch of {B}")
        latents = self.prepare_latents(video, ts[:1], generator=generator, latents=latents)
        num_frames = latents.shape[2]
        local = latents
        if self.dist is not None:  # every rank computed the same latents from the shared CPU generator
            fl = self.dist.frames_local(num_frames)
            local = latents[:, :, self.dist.rank * fl:(self.dist.rank + 1) * fl]
        if self.free_init_enabled:
            out = self._free_init_sample(
                latents, num_inference_steps, generator,
                lambda t: DenoiseLoop(self.unet, self.scheduler, latents, ehs, guidance_scale, timesteps=t,
                                      use_graph=use_graph, ip_embeds=ip_embeds,
                                      step_noise=self._step_noise(latents, len(t), None, draw=False)),
                schedule=lambda t: self.get_timesteps(len(t), strength)[0])
        else:
            step_noise = self._step_noise(latents, len(ts), generator)  # after prepare_latents' draws
            loop = DenoiseLoop(self.unet, self.scheduler, local, ehs, guidance_scale, timesteps=ts,
                               use_graph=use_graph, ip_embeds=ip_embeds, step_noise=step_noise).prime()
            out = loop.run()
        if self.dist is not None:
            out = self.dist.all_gather_frames(out)
        if output_type != "latent":
            out = self.postprocess_video(self.decode_latents(out), output_type)
        return AnimateDiffPipelineOutput(frames=out) if return_dict else (out,)


class AnimateDiffControlNetPipeline(AnimateDiffPipeline):
    """diffusers AnimateDiffControlNetPipeline: `pipe(prompt=, conditioning_frames=, ...)` runs the
    text-to-video pipeline's loop with a ControlNet on every step's input, inside the same
    captured graph (DenoiseLoop(control=)).  IP-Adapter, FreeU, FreeNoise, LoRA and the LCM
    scheduler combine with it as they do with the plain pipeline.  Refused: a list of ControlNets
    (MultiControlNet), a frame-sharded pipeline (dist=), FreeInit.  Parity to diffusers is
    unpinned, as the UNet's."""

    def __init__(self, unet, controlnet, scheduler=None, text_encoder=None, vae=None, dist=None, tokenizer=None):
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError("a list of ControlNets (MultiControlNetModel) is not supported: pass one")
        if not isinstance(controlnet, ControlNetModel):
            raise ValueError("AnimateDiffControlNetPipeline needs controlnet=vdiff.ControlNetModel(...)")
        if dist is not None:
            raise NotImplementedError("AnimateDiffControlNetPipeline with a frame-sharded pipeline (dist=) is not "
                                      "supported: the ControlNet's residuals are not sharded over the ranks' frames")
        super().__init__(unet, scheduler, text_encoder=text_encoder, vae=vae, dist=dist, tokenizer=tokenizer)
        self.controlnet = controlnet
        self._control = None  # the running call's ControlNetConditioning arguments

    @classmethod
    def from_config(cls, config="full", device="cuda", seed=0, scheduler=None, dist=None, vae="auto",
                    controlnet_seed=1):
        """Synthetic-weight pipeline: AnimateDiffPipeline.from_config's, plus a synthetic ControlNet
        of the same config (its zero convs are NOT zero, or it would be invisible)."""
        base = AnimateDiffPipeline.from_config(config, device=device, seed=seed, scheduler=scheduler, dist=None,
                                               vae=vae)
        cn = init_synthetic_(ControlNetModel(config), controlnet_seed).to(device=device, dtype=torch.bfloat16)
        pipe = cls(base.unet, cn.prepare(), base.scheduler, vae=base.vae, dist=dist)
        pipe.torch_dtype = base.torch_dtype
        return pipe

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, controlnet=None, motion_adapter=None, **kwargs):
        """AnimateDiffPipeline.from_pretrained's components plus controlnet=ControlNetModel.from_pretrained(...)."""
        if controlnet is None:
            raise ValueError("AnimateDiffControlNetPipeline needs controlnet=ControlNetModel.from_pretrained(...)")
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError("a list of ControlNets (MultiControlNetModel) is not supported: pass one")
        if kwargs.get("dist") is not None:
            raise NotImplementedError("AnimateDiffControlNetPipeline with a frame-sharded pipeline (dist=) is not "
                                      "supported")
        base = AnimateDiffPipeline.from_pretrained(pretrained_model_name_or_path, motion_adapter=motion_adapter,
                                                   **kwargs)
        if controlnet.device.type == "cuda":
            controlnet.prepare()
        pipe = cls(base.unet, controlnet, base.scheduler, vae=base.vae, tokenizer=base.tokenizer,
                   text_encoder=base.text_encoder if base.tokenizer is not None else None)
        pipe.torch_dtype = base.torch_dtype
        return pipe

    def _make_loop(self, unet, scheduler, latents, *args, **kwargs):
        c = self._control
        control = ControlNetConditioning(self.controlnet, c["frames"], c["scale"], c["guess_mode"], c["start"],
                                         c["end"])
        return DenoiseLoop(unet, scheduler, latents, *args, control=control, **kwargs)

    @torch.no_grad()
    def __call__(self, prompt=None, num_frames=16, height=None, width=None, num_inference_steps=50,
                 guidance_scale=7.5, *, conditioning_frames=None, controlnet_conditioning_scale=1.0,
                 guess_mode=False, control_guidance_start=0.0, control_guidance_end=1.0, **kwargs):
        if self.free_init_enabled:
            raise NotImplementedError("FreeInit together with ControlNet is not supported: the guidance window is "
                                      "laid out over one schedule, FreeInit runs several; disable_free_init()")
        if self.dist is not None:
            raise NotImplementedError("AnimateDiffControlNetPipeline with a frame-sharded pipeline (dist=) is not "
                                      "supported")
        if conditioning_frames is None:
            raise ValueError("conditioning_frames required: one control image per frame")
        for v in (controlnet_conditioning_scale, control_guidance_start, control_guidance_end):
            if isinstance(v, (list, tuple)):
                raise NotImplementedError("per-ControlNet lists of scales / guidance windows (MultiControlNet) are "
                                          "not supported")
        sample = self.unet.config["sample_size"]
        height, width = height or sample * 8, width or sample * 8
        frames = decode_video_frames(conditioning_frames, height, width).permute(0, 2, 1, 3, 4).contiguous()
        if frames.shape[2] != num_frames:
            raise ValueError(f"{frames.shape[2]} conditioning frames for num_frames={num_frames}")
        if tuple(frames.shape[3:]) != (height, width):
            raise ValueError(f"conditioning frames are {frames.shape[3]} x {frames.shape[4]}, the video "
                             f"{height} x {width}")
        control_scale_table(1, 1, controlnet_conditioning_scale, guess_mode, control_guidance_start,
                            control_guidance_end)  # refuses a bad guidance window before any work
        self._control = dict(frames=frames, scale=controlnet_conditioning_scale, guess_mode=guess_mode,
                             start=control_guidance_start, end=control_guidance_end)
        try:
            return super().__call__(prompt=prompt, num_frames=num_frames, height=height, width=width,
                                    num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, **kwargs)
        finally:
            self._control = None


def decode_key_frames(frames, height=None, width=None):
    """SparseCtrl's conditioning_frames -> (K, 3, H, W) fp32 in [0, 1] on the CPU: a list of PIL
    images, a list of (H, W, 3) arrays or (3, H, W) tensors, an (K, H, W, 3) array or an (K, 3, H, W)
    tensor; one image alone is K = 1.  PIL images of another size than height x width are resized,
    arrays and tensors refused (decode_video_frames)."""
    import numpy as np
    if isinstance(frames, (list, tuple)) and len(frames) > 0:
        if isinstance(frames[0], np.ndarray):
            frames = np.stack([np.asarray(f) for f in frames])
        elif torch.is_tensor(frames[0]):
            frames = torch.stack(list(frames))
    elif not isinstance(frames, (list, tuple, np.ndarray)) and not torch.is_tensor(frames):
        frames = [frames]  # one PIL image
    x = decode_video_frames(frames, height, width)
    if x.shape[0] != 1:
        raise ValueError("conditioning_frames: one list of key frames (per-video key frames are not supported)")
    return x[0]


class AnimateDiffSparseControlNetPipeline(AnimateDiffPipeline):
    """diffusers AnimateDiffSparseControlNetPipeline (SparseCtrl): `pipe(prompt=, conditioning_frames=,
    controlnet_frame_indices=[0, 8, 15], ...)` conditions the video on a few key frames.  The key
    frames — VAE latents for an RGB checkpoint (use_simplified_condition_embedding), the [0, 1]
    images for a scribble one — become the condition rows with their mask column in one launch
    (ops.sparse_cond), the conditioning embedding runs once per call, and a SparseControlNetModel,
    which reads no latents, runs inside the captured graph of every step (DenoiseLoop(control=)).
    IP-Adapter, FreeU, LoRA and the DDIM, Euler, LCM and DPM schedulers combine with it as with the
    plain pipeline.  Refused: a list of ControlNets, dist=, cfg_shard, FreeInit, FreeNoise.
    Parity to diffusers is unpinned, as the UNet's."""

    vae_encoder = True  # from_config: the RGB variant encodes its key frames

    def __init__(self, unet, controlnet, scheduler=None, text_encoder=None, vae=None, dist=None, tokenizer=None):
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError("a list of ControlNets (MultiControlNetModel) is not supported: pass one")
        if not isinstance(controlnet, SparseControlNetModel):
            raise ValueError("AnimateDiffSparseControlNetPipeline needs controlnet=vdiff.SparseControlNetModel(...)")
        if dist is not None:
            raise NotImplementedError("AnimateDiffSparseControlNetPipeline with a frame-sharded pipeline (dist=) is "
                                      "not supported: the ControlNet's motion modules need every frame of a video")
        super().__init__(unet, scheduler, text_encoder=text_encoder, vae=vae, dist=dist, tokenizer=tokenizer)
        self.controlnet = controlnet
        self._control = None  # the running call's SparseControlConditioning arguments

    @classmethod
    def from_config(cls, config="full", device="cuda", seed=0, scheduler=None, dist=None, vae="auto",
                    controlnet_seed=1, use_simplified_condition_embedding=True):
        """Synthetic-weight pipeline: AnimateDiffPipeline.from_config's with the VAE's encoder, plus
        a synthetic SparseControlNetModel of the same config (its zero convs are NOT zero, or it
        would be invisible)."""
        if dist is not None:
            raise NotImplementedError("AnimateDiffSparseControlNetPipeline with a frame-sharded pipeline (dist=) is "
                                      "not supported")
        base = AnimateDiffPipeline.from_config(config, device=device, seed=seed, scheduler=scheduler, vae=None)
        if vae == "auto":
            vae = config if config in ("tiny", "full") else None
        if isinstance(vae, str):
            vae = init_synthetic_(AutoencoderKL(vae, encoder=True), seed).to(device=device, dtype=torch.bfloat16).prepare()
        base.vae = vae
        extra = {} if use_simplified_condition_embedding else dict(use_simplified_condition_embedding=False,
                                                                   conditioning_channels=3)
        cn = init_synthetic_(SparseControlNetModel(config, **extra), controlnet_seed)
        cn = cn.to(device=device, dtype=torch.bfloat16)
        pipe = cls(base.unet, cn.prepare(), base.scheduler, vae=base.vae)
        pipe.torch_dtype = base.torch_dtype
        return pipe

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, controlnet=None, motion_adapter=None, **kwargs):
        """AnimateDiffPipeline.from_pretrained's components plus
        controlnet=SparseControlNetModel.from_pretrained(...)."""
        if controlnet is None:
            raise ValueError("AnimateDiffSparseControlNetPipeline needs "
                             "controlnet=SparseControlNetModel.from_pretrained(...)")
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError("a list of ControlNets (MultiControlNetModel) is not supported: pass one")
        if kwargs.get("dist") is not None:
            raise NotImplementedError("AnimateDiffSparseControlNetPipeline with a frame-sharded pipeline (dist=) is "
                                      "not supported")
        base = AnimateDiffPipeline.from_pretrained(pretrained_model_name_or_path, motion_adapter=motion_adapter,
                                                   **kwargs)
        if controlnet.device.type == "cuda":
            controlnet.prepare()
        pipe = cls(base.unet, controlnet, base.scheduler, vae=base.vae, tokenizer=base.tokenizer,
                   text_encoder=base.text_encoder if base.tokenizer is not None else None)
        pipe.torch_dtype = base.torch_dtype
        return pipe

    # ------------------------------------------------------------------ the condition
    def _sparse_rows(self, key_frames, num_frames, controlnet_frame_indices):
        """key_frames (B, C, K, h, w) -> ops.sparse_cond's rows [B * num_frames * h * w, 8]."""
        cc = self.controlnet.config["conditioning_channels"]
        if key_frames.dim() != 5 or key_frames.shape[1] != cc:
            raise ValueError(f"key frames of shape {tuple(key_frames.shape)}: expected (B, {cc}, K, h, w)")
        idx = list(controlnet_frame_indices)
        B, _, K, h, w = key_frames.shape
        if len(idx) > K:
            raise ValueError(f"{len(idx)} controlnet_frame_indices for {K} conditioning frames")
        ops.sparse_frame_indices(idx, num_frames)  # IndexError before any device work
        keys = key_frames[:, :, :len(idx)].to(self.unet.device, torch.float32).contiguous()
        rows = ops.pack_latents(keys, dup=1, cpad=CIN_PAD)
        return ops.sparse_cond(rows, idx, B, num_frames, h * w, cc)

    @torch.no_grad()
    def prepare_sparse_control_conditioning(self, conditioning_frames, num_frames, controlnet_frame_indices,
                                            device=None, dtype=None):
        """diffusers' method of that name: conditioning_frames (B, C, K, h, w), K >= len(indices) —
        VAE latents x scaling_factor for the simplified embedding, [0, 1] images for the full one —
        -> (controlnet_cond (B, C, F, h, w), conditioning_mask (B, 1, F, h, w)), fp32: zeros, the
        first len(indices) key frames at their frame indices, the mask 1 there.  One launch of
        vd_rows_eltwise op 8 builds both."""
        B, C, _, h, w = conditioning_frames.shape
        rows = self._sparse_rows(conditioning_frames, num_frames, controlnet_frame_indices)
        both = ops.unpack_nhwc(rows, B, C + 1, num_frames, h, w)
        cond, mask = both[:, :C].contiguous(), both[:, C:].contiguous()
        if device is not None or dtype is not None:
            cond, mask = cond.to(device=device, dtype=dtype), mask.to(device=device, dtype=dtype)
        return cond, mask

    @torch.no_grad()
    def prepare_key_frames(self, images, h, w, generator=None):
        """(K, 3, H, W) images in [0, 1] -> the key frames (1, C, K, h', w') the ControlNet's
        embedding takes for h x w latents: the VAE latents x scaling_factor of 2 x - 1 (simplified
        embedding; the posterior is sampled with the call's generator), or the images themselves."""
        cn = self.controlnet
        if cn.simplified:
            if self.vae is None or getattr(self.vae, "encoder", None) is None:
                raise ValueError("a SparseControlNetModel with use_simplified_condition_embedding conditions on the "
                                 "VAE latents of the key frames: AnimateDiffSparseControlNetPipeline needs a VAE "
                                 "with its encoder, AutoencoderKL(config, encoder=True)")
            x = (2.0 * images - 1.0).to(self.unet.device)
            n = self.vae.frames_per_chunk
            lat = torch.cat([self.vae.encode(x[i:i + n]).latent_dist.sample(generator=generator)
                             for i in range(0, x.shape[0], n)]) * self.vae.config["scaling_factor"]
            if tuple(lat.shape[1:]) != (cn.config["conditioning_channels"], h, w):
                raise ValueError(f"the key frames encode to {tuple(lat.shape[1:])} latents, the video's are "
                                 f"({cn.config['conditioning_channels']}, {h}, {w}): resize the conditioning frames")
            return lat.permute(1, 0, 2, 3)[None].float()
        if tuple(images.shape[1:]) != (cn.config["conditioning_channels"], 8 * h, 8 * w):
            raise ValueError(f"conditioning frames are {tuple(images.shape[1:])}, the video needs "
                             f"({cn.config['conditioning_channels']}, {8 * h}, {8 * w})")
        return images.permute(1, 0, 2, 3)[None].float()

    def _make_loop(self, unet, scheduler, latents, *args, **kwargs):
        c = self._control
        if kwargs.get("cfg_shard") is not None:
            raise NotImplementedError("AnimateDiffSparseControlNetPipeline with cfg_shard is not supported")
        control = SparseControlConditioning(self.controlnet, c["rows"], *c["geometry"], c["scale"], c["guess_mode"])
        return DenoiseLoop(unet, scheduler, latents, *args, control=control, **kwargs)

    @torch.no_grad()
    def __call__(self, prompt=None, num_frames=16, height=None, width=None, num_inference_steps=50,
                 guidance_scale=7.5, *, conditioning_frames=None, controlnet_conditioning_scale=1.0,
                 controlnet_frame_indices=(0,), guess_mode=False, generator=None, cfg_shard=None, **kwargs):
        if self.free_init_enabled:
            raise NotImplementedError("FreeInit together with SparseCtrl is not supported; disable_free_init()")
        if self.free_noise_enabled:
            raise NotImplementedError("FreeNoise together with SparseCtrl is not supported: the ControlNet's own "
                                      "motion modules would need the windows too; disable_free_noise()")
        if self.dist is not None:
            raise NotImplementedError("AnimateDiffSparseControlNetPipeline with a frame-sharded pipeline (dist=) is "
                                      "not supported")
        if cfg_shard is not None:
            raise NotImplementedError("AnimateDiffSparseControlNetPipeline with cfg_shard is not supported")
        if conditioning_frames is None:
            raise ValueError("conditioning_frames required: the key frames")
        if isinstance(controlnet_conditioning_scale, (list, tuple)):
            raise NotImplementedError("a list of conditioning scales (MultiControlNet) is not supported")
        mlen = self.controlnet.config["motion_max_seq_length"]
        if num_frames > mlen:
            raise ValueError(f"num_frames={num_frames} exceeds the SparseControlNetModel's motion_max_seq_length={mlen}")
        sample = self.unet.config["sample_size"]
        height, width = height or sample * 8, width or sample * 8
        h, w = height // 8, width // 8
        idx = list(controlnet_frame_indices)
        ops.sparse_frame_indices(idx, num_frames)
        # the size the embedding needs: 8 x the latents for images, the VAE's own factor for latents
        ds = 8
        if self.controlnet.simplified and self.vae is not None:
            ds = 2 ** (len(self.vae.config["block_out_channels"]) - 1)
        images = decode_key_frames(conditioning_frames, ds * h, ds * w)
        if len(idx) > images.shape[0]:
            raise ValueError(f"{len(idx)} controlnet_frame_indices for {images.shape[0]} conditioning frames")
        keys = self.prepare_key_frames(images[:len(idx)], h, w, generator=generator)
        rows = self._sparse_rows(keys, num_frames, idx)
        self._control = dict(rows=rows, geometry=(1, num_frames, keys.shape[3], keys.shape[4]),
                             scale=float(controlnet_conditioning_scale), guess_mode=bool(guess_mode))
        try:
            return super().__call__(prompt=prompt, num_frames=num_frames, height=height, width=width,
                                    num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                    generator=generator, **kwargs)
        finally:
            self._control = None


class AnimateDiffPAGPipeline(AnimateDiffPipeline):
    """diffusers AnimateDiffPAGPipeline (PAGMixin): perturbed-attention guidance.  Every step runs
    one more branch through the UNet in which the self-attentions selected by pag_applied_layers
    use an identity attention map (their output is the V projection), and the step kernel adds
    pag_scale * (eps_cond - eps_perturbed) to the (CFG-combined) eps: DenoiseLoop(pag=).  Layer ids
    follow diffusers: regular expressions searched in the attention modules' names, self-attentions
    only, so the default "mid_block.*attn1" selects the mid block's spatial attn1 and its motion
    module's attn1.  It runs with all four schedulers, FreeU, FreeInit, LoRA and IP-Adapter.
    Refused: a frame-sharded pipeline (dist=), FreeNoise; DenoiseLoop also refuses cfg_shard and
    ControlNet.  With pag_scale = 0 (or no layers) a call is AnimateDiffPipeline's, untouched.
    Parity to diffusers is unpinned (diffusers is not a dependency); tests/pag_ref.py restates it."""

    def __init__(self, unet, scheduler=None, text_encoder=None, vae=None, dist=None, tokenizer=None,
                 pag_applied_layers="mid_block.*attn1"):
        super().__init__(unet, scheduler, text_encoder=text_encoder, vae=vae, dist=dist, tokenizer=tokenizer)
        self._pag_scale, self._pag_adaptive_scale = 3.0, 0.0
        self.set_pag_applied_layers(pag_applied_layers)

    @classmethod
    def from_config(cls, config="full", device="cuda", seed=0, scheduler=None, dist=None, vae="auto",
                    pag_applied_layers="mid_block.*attn1"):
        base = AnimateDiffPipeline.from_config(config, device=device, seed=seed, scheduler=scheduler, dist=dist, vae=vae)
        pipe = cls(base.unet, base.scheduler, vae=base.vae, dist=dist, pag_applied_layers=pag_applied_layers)
        pipe.torch_dtype = base.torch_dtype
        return pipe

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, motion_adapter=None,
                        pag_applied_layers="mid_block.*attn1", **kwargs):
        base = AnimateDiffPipeline.from_pretrained(pretrained_model_name_or_path, motion_adapter=motion_adapter,
                                                   **kwargs)
        pipe = cls(base.unet, base.scheduler, vae=base.vae, dist=base.dist, tokenizer=base.tokenizer,
                   text_encoder=base.text_encoder if base.tokenizer is not None else None,
                   pag_applied_layers=pag_applied_layers)
        pipe.torch_dtype = base.torch_dtype
        return pipe

    def set_pag_applied_layers(self, pag_applied_layers):
        """diffusers' PAGMixin.set_pag_applied_layers: a layer id or a list of them (strings); the
        UNet's matching self-attentions are marked at once, and an id that matches none raises
        ValueError (diffusers raises it at the first call)."""
        layers = [pag_applied_layers] if isinstance(pag_applied_layers, str) else list(pag_applied_layers or [])
        if not all(isinstance(x, str) for x in layers):
            raise ValueError(f"pag_applied_layers must be a string or a list of strings, got {pag_applied_layers!r}")
        self.unet.set_pag_applied_layers(layers)
        self.pag_applied_layers = layers

    @property
    def pag_scale(self) -> float:
        return self._pag_scale

    @property
    def pag_adaptive_scale(self) -> float:
        return self._pag_adaptive_scale

    @property
    def do_pag_adaptive_scaling(self) -> bool:
        return self._pag_adaptive_scale > 0 and self._pag_scale > 0 and len(self.pag_applied_layers) > 0

    @property
    def do_perturbed_attention_guidance(self) -> bool:
        return self._pag_scale > 0 and self._pag_adaptive_scale >= 0 and len(self.pag_applied_layers) > 0

    def _make_loop(self, unet, scheduler, latents, ehs, guidance_scale, ip_embeds=None, **kwargs):
        if not self.do_perturbed_attention_guidance:
            return DenoiseLoop(unet, scheduler, latents, ehs, guidance_scale, ip_embeds=ip_embeds, **kwargs)
        # the perturbed branch takes the conditional embeddings: [neg, pos, pos] or [pos, pos]
        B = latents.shape[0]
        ehs = torch.cat([ehs, ehs[-B:]])
        if ip_embeds is not None:
            ip_embeds = torch.cat([ip_embeds, ip_embeds[-B:]])
        # another pipeline on the same UNet may have marked other layers since
        unet.set_pag_applied_layers(self.pag_applied_layers)
        pag = PerturbedAttentionGuidance(self._pag_scale, self._pag_adaptive_scale)
        return DenoiseLoop(unet, scheduler, latents, ehs, guidance_scale, ip_embeds=ip_embeds, pag=pag, **kwargs)

    @torch.no_grad()
    def __call__(self, *args, pag_scale: float = 3.0, pag_adaptive_scale: float = 0.0, **kwargs):
        self._pag_scale, self._pag_adaptive_scale = float(pag_scale), float(pag_adaptive_scale)
        if self.do_perturbed_attention_guidance:
            if self.dist is not None:
                raise NotImplementedError("AnimateDiffPAGPipeline with a frame-sharded pipeline (dist=) is not "
                                          "supported: the perturbed branch is whole videos of one rank's UNet batch")
            if self.free_noise_enabled:
                raise NotImplementedError("perturbed-attention guidance with FreeNoise is not supported: the windows "
                                          "ride on the batch axis of the temporal kernels; disable_free_noise()")
        return super().__call__(*args, **kwargs)
