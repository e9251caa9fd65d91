"""SparseControlNetModel — diffusers:SparseControlNetModel (SparseCtrl) for SD-1.5 + AnimateDiff on
MI355X: the UNet's encoder half WITH its motion modules, a conditioning embedding in front and
one 1x1 "zero" conv behind every skip and the mid block.  A few key frames condition the whole
video: the condition tensor holds the key frames at their frame indices, zeros elsewhere, and one
extra mask channel that is 1 on the conditioned frames; the motion modules carry a condition at
frame 0 to frame 15.  State-dict names are diffusers', so a published SparseCtrl folder loads
through `SparseControlNetModel.from_pretrained(local_dir)`.

The model never reads the latents (diffusers: `sample = torch.zeros_like(sample)`), so
`conv_in(sample)` is `conv_in.bias`: it is folded on the host into the bias of the embedding's
last conv, `embed_condition` returns the whole input of down block 0 — once per video, it depends
on no timestep — and `forward_rows` takes no latent rows and launches no conv_in.

Compute: the existing kernels.  The down blocks are the UNet's CrossAttnDownBlockMotion /
DownBlockMotion, the mid block ControlNetModel's, the condition rows come from vd_rows_eltwise
op 8 (ops.sparse_cond), the residuals leave `forward_rows` unscaled as ControlNetModel's do.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..config import down_block_plan, get_config
from .blocks import CrossAttnDownBlockMotion, Ctx, DownBlockMotion, ResnetBlock2D
from .controlnet import (ControlNetConditioningEmbedding, ControlNetModel, ControlNetOutput, UNetMidBlock2DCrossAttn,
                         guess_mode_scales)
from .layers import Act, Conv2d, TimestepEmbedding, Timesteps, bf, f32, rows_fmap
from .unet_motion import CIN_PAD, FrozenDict

# what a SparseCtrl config adds to the UNet config it shares its encoder with
SPARSE_CONTROLNET_FULL = dict(conditioning_channels=4, conditioning_embedding_out_channels=(16, 32, 96, 256),
                              concat_conditioning_mask=True, use_simplified_condition_embedding=True)
SPARSE_CONTROLNET_TINY = dict(conditioning_channels=4, conditioning_embedding_out_channels=(16, 32, 32, 64),
                              concat_conditioning_mask=True, use_simplified_condition_embedding=True)
_EXTRA = {"full": SPARSE_CONTROLNET_FULL, "tiny": SPARSE_CONTROLNET_TINY}
_DOWN_MOTION = ("CrossAttnDownBlockMotion", "DownBlockMotion")


def sparse_controlnet_config(name_or_cfg, **overrides) -> dict:
    """The UNet config of that name (vdiff.config), its motion modules kept, plus SparseCtrl's own
    entries; `overrides` replace entries (use_simplified_condition_embedding=False, ...)."""
    cfg = get_config(name_or_cfg)
    extra = SPARSE_CONTROLNET_FULL if isinstance(name_or_cfg, dict) else _EXTRA[name_or_cfg]
    for k, v in extra.items():
        if isinstance(name_or_cfg, dict):
            cfg.setdefault(k, v)
        else:
            cfg[k] = v
    cfg.update(overrides)
    cfg["conditioning_embedding_out_channels"] = tuple(cfg["conditioning_embedding_out_channels"])
    cfg["down_block_types"] = tuple(cfg["down_block_types"])
    for k in ("up_block_types", "out_channels", "use_motion_mid_block"):
        cfg.pop(k, None)
    if any(t not in _DOWN_MOTION for t in cfg["down_block_types"]):
        raise NotImplementedError(f"down_block_types {cfg['down_block_types']}: only {_DOWN_MOTION} are built")
    if not cfg["concat_conditioning_mask"]:
        raise NotImplementedError("concat_conditioning_mask=False is not built: the condition rows always carry "
                                  "their mask column")
    if not 1 <= cfg["conditioning_channels"] <= 7:
        raise NotImplementedError(f"conditioning_channels={cfg['conditioning_channels']}: the packed condition rows "
                                  "hold 1..7 channels and the mask")
    return cfg


class SparseControlNetModel(nn.Module):
    reads_latents = False  # DenoiseLoop: forward_rows takes the condition rows alone

    def __init__(self, config="full", **overrides):
        super().__init__()
        cfg = sparse_controlnet_config(config, **overrides)
        self.config = FrozenDict(cfg)
        boc = cfg["block_out_channels"]
        g, eps = cfg["norm_num_groups"], cfg["norm_eps"]
        heads, mheads = cfg["num_attention_heads"], cfg["motion_num_attention_heads"]
        cross, mlen = cfg["cross_attention_dim"], cfg["motion_max_seq_length"]
        tdim = boc[0] * 4
        self.conv_in = Conv2d(cfg["in_channels"], boc[0], 3, padding=1)
        self.time_proj = Timesteps(boc[0])
        self.time_embedding = TimestepEmbedding(boc[0], tdim)
        cin = cfg["conditioning_channels"] + 1  # the mask channel
        if cfg["use_simplified_condition_embedding"]:
            self.controlnet_cond_embedding = Conv2d(cin, boc[0], 3, padding=1)
        else:
            self.controlnet_cond_embedding = ControlNetConditioningEmbedding(
                boc[0], cin, cfg["conditioning_embedding_out_channels"])
        self.down_blocks = nn.ModuleList()
        self.controlnet_down_blocks = nn.ModuleList([Conv2d(boc[0], boc[0], 1)])
        for (out_ch, ins, has_attn, down) in down_block_plan(cfg):
            if has_attn:
                blk = CrossAttnDownBlockMotion(ins[0], out_ch, tdim, len(ins), heads, cross, mheads, down, g, eps, mlen)
            else:
                blk = DownBlockMotion(ins[0], out_ch, tdim, len(ins), mheads, down, g, eps, mlen)
            self.down_blocks.append(blk)
            for _ in range(len(ins) + int(down)):
                self.controlnet_down_blocks.append(Conv2d(out_ch, out_ch, 1))
        self.controlnet_mid_block = Conv2d(boc[-1], boc[-1], 1)
        self.mid_block = UNetMidBlock2DCrossAttn(boc[-1], tdim, heads, cross, g, eps)
        self._prepared = False

    # ------------------------------------------------------------------ utils
    dtype = ControlNetModel.dtype
    device = ControlNetModel.device
    num_residuals = ControlNetModel.num_residuals
    residual_channels = ControlNetModel.residual_channels
    resnets_in_order = ControlNetModel.resnets_in_order
    make_ctx = ControlNetModel.make_ctx

    @property
    def simplified(self) -> bool:
        return bool(self.config["use_simplified_condition_embedding"])

    @property
    def condition_downscale(self) -> int:
        """Condition pixels per latent pixel: 1 for the simplified embedding (the condition is a
        VAE latent), 8 for the full one (the condition is an image)."""
        return 1 if self.simplified else 8

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=None, variant=None, device="cuda", **unused):
        """diffusers SparseControlNetModel.from_pretrained over a LOCAL folder (config.json +
        diffusion_pytorch_model[.variant].safetensors), bf16 on `device`."""
        from .. import pretrained as P
        if isinstance(pretrained_model_name_or_path, (list, tuple)):
            raise NotImplementedError("a list of ControlNets (MultiControlNetModel) is not supported: load one")
        d = P._local_dir(pretrained_model_name_or_path, "SparseControlNetModel.from_pretrained")
        cfg = sparse_controlnet_config_from_diffusers(P.read_json(d / "config.json"))
        m = P._assign(P._empty_on(cls, cfg, device), P.load_weights(d, variant), what="SparseControlNetModel")
        m.torch_dtype = torch_dtype
        return m

    @torch.no_grad()
    def prepare(self):
        """Pack device operands for the HIP kernels (idempotent; re-run after a weight load)."""
        if not next(self.parameters()).is_cuda:
            raise RuntimeError("SparseControlNetModel.prepare(): move the model to the GPU first (no CPU path)")
        for m in self.modules():
            if m is not self and hasattr(m, "prepare"):
                m.prepare()
        last = self._embed_convs()[-1]
        assert self._embed_convs()[0]._cin_pad == CIN_PAD
        # conv_in(zeros) is conv_in.bias: one fp32 bias for the embedding's last conv
        self._b_embed = f32(last.bias.float() + self.conv_in.bias.float())
        res = self.resnets_in_order()
        off = 0
        for r in res:  # offsets into this model's own concatenated time_emb_proj table, as ControlNetModel.prepare
            r.temb_offset = off
            off += r.out_channels
        self._w_temb = bf(torch.cat([r.time_emb_proj.weight for r in res], 0))
        self._b_temb = f32(torch.cat([r.time_emb_proj.bias for r in res], 0))
        self._prepared = True
        return self

    # ------------------------------------------------------------------ core
    def _embed_convs(self):
        e = self.controlnet_cond_embedding
        return [e] if self.simplified else e.convs()

    def _check_frames(self, frames):
        mlen = self.config["motion_max_seq_length"]
        if frames > mlen:
            raise ValueError(f"SparseControlNetModel: {frames} frames exceed motion_max_seq_length={mlen}: the "
                             "ControlNet's motion modules run over the whole video (the temporal kernels end there)")

    @torch.no_grad()
    def embed_condition(self, cond_rows, n_img, h, w):
        """The packed condition rows [n_img * h * w, 8] of ops.sparse_cond (h x w the CONDITION's
        size: the latent's for the simplified embedding, 8 x that for the full one) -> the bf16
        NHWC rows [n_img * h' * w', C0] of down block 0's input, `conv_in(0) + embedding(cond)`.
        It depends on no timestep and no latent: the pipeline computes it once per video.  Frames
        are chunked where one launch's activation would pass vd_gemm's 2^31-element bound."""
        if not self._prepared:
            self.prepare()
        if cond_rows.shape[0] != n_img * h * w or cond_rows.shape[1] != CIN_PAD:
            raise ValueError(f"embed_condition: rows of shape {tuple(cond_rows.shape)} are not {n_img} images of "
                             f"{h} x {w} in {CIN_PAD} columns")
        convs = self._embed_convs()
        ds = self.condition_downscale
        if h % ds or w % ds:
            raise ValueError(f"conditioning frames must be multiples of {ds} in height and width, got {h} x {w}")
        per, hh, ww = h * w * CIN_PAD, h, w
        for c in convs:
            hh, ww = (hh - 1) // c.stride[0] + 1, (ww - 1) // c.stride[0] + 1
            per = max(per, hh * ww * c.out_channels)
        if per >= 0x7fffffff:
            raise ValueError(f"one {h} x {w} conditioning frame exceeds the conv kernels' 2^31-element bound")
        chunk = max(1, (0x7fffffff - 1) // per)
        ho, wo = h // ds, w // ds
        out = torch.empty(n_img * ho * wo, convs[-1].out_channels, device=cond_rows.device, dtype=torch.bfloat16)
        for f0 in range(0, n_img, chunk):
            n = min(chunk, n_img - f0)
            rows, hh, ww = cond_rows[f0 * h * w:(f0 + n) * h * w], h, w
            for i, c in enumerate(convs):
                last = i == len(convs) - 1
                rows, hh, ww = ops.conv3x3(rows, n, hh, ww, c._w, stride=c.stride[0],
                                           bias=self._b_embed if last else c._b,
                                           act=ops.ACT_NONE if last else ops.ACT_SILU)
            out[f0 * ho * wo:(f0 + n) * ho * wo].copy_(rows)
        return out

    def forward_rows(self, emb_rows, h, w, ctx: Ctx):
        """embed_condition's rows of the ctx.batch videos of ctx.frames frames -> the UNscaled
        zero-conv outputs as Acts: one per UNet skip, then the mid one.  No latent rows."""
        self._check_frames(ctx.frames)
        n_img = ctx.batch * ctx.frames
        if emb_rows.shape[0] != n_img * h * w:
            raise ValueError(f"{emb_rows.shape[0]} embedded condition rows for {n_img} frames of {h} x {w}")
        x = Act(emb_rows, n_img, h, w)
        outs = [x]
        for blk in self.down_blocks:
            x, o = blk.run(x, ctx)
            outs.extend(o)
        outs.append(self.mid_block.run(x, ctx))
        zero = [*self.controlnet_down_blocks, self.controlnet_mid_block]
        return [Act(ops.gemm(a.t, z._w, bias=z._b), a.n, a.h, a.w) for a, z in zip(outs, zero)]

    def condition_rows(self, controlnet_cond, conditioning_mask):
        """diffusers' (B, C, F, h, w) condition and (B, 1, F, h, w) mask -> the packed rows
        [B * F * h * w, 8] `cat([cond, mask], 1)` stands for (columns above the mask zero)."""
        cc = self.config["conditioning_channels"]
        if controlnet_cond.dim() != 5 or controlnet_cond.shape[1] != cc:
            raise ValueError(f"controlnet_cond: expected (B, {cc}, F, h, w), got {tuple(controlnet_cond.shape)}")
        B, _, Fr, h, w = controlnet_cond.shape
        if tuple(conditioning_mask.shape) != (B, 1, Fr, h, w):
            raise ValueError(f"conditioning_mask of shape {tuple(conditioning_mask.shape)}: expected {(B, 1, Fr, h, w)}")
        dev = self.device
        both = torch.cat([controlnet_cond.to(dev).float(), conditioning_mask.to(dev).float()], 1).contiguous()
        return ops.pack_latents(both, dup=1, cpad=CIN_PAD)

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_mask=None,
                conditioning_scale=1.0, timestep_cond=None, attention_mask=None, cross_attention_kwargs=None,
                guess_mode: bool = False, return_dict: bool = True):
        """diffusers SparseControlNetModel.forward: sample (B, C, F, H, W) — only its shape is
        used —, encoder_hidden_states (B, L, D) or (1, L, D), controlnet_cond (B, cc, F, h, w) and
        conditioning_mask (B, 1, F, h, w), h x w the latent's size (simplified embedding) or 8 x
        it -> ControlNetOutput of (B * F, C_i, H_i, W_i) bf16 residuals times conditioning_scale
        (times logspace(-1, 0, n) in guess mode)."""
        if not self._prepared:
            self.prepare()
        for unsupported, name in ((timestep_cond, "timestep_cond"), (attention_mask, "attention_mask")):
            if unsupported is not None:
                raise NotImplementedError(f"{name} is not supported by this SparseControlNetModel")
        if isinstance(conditioning_scale, (list, tuple)):
            raise NotImplementedError("a list of conditioning scales (MultiControlNetModel) is not supported")
        if sample.dim() != 5:
            raise ValueError(f"sample: expected (batch, C, frames, H, W), got {tuple(sample.shape)}")
        if conditioning_mask is None:
            raise ValueError("conditioning_mask required (concat_conditioning_mask=True)")
        dev = self.device
        B, _, Fr, H, W = sample.shape
        self._check_frames(Fr)
        ds = self.condition_downscale
        if controlnet_cond.dim() != 5 or tuple(controlnet_cond.shape[0:1] + controlnet_cond.shape[2:]) != \
                (B, Fr, ds * H, ds * W):
            raise ValueError(f"controlnet_cond of shape {tuple(controlnet_cond.shape)}: expected ({B}, "
                             f"{self.config['conditioning_channels']}, {Fr}, {ds * H}, {ds * W})")
        t = torch.as_tensor(timestep, device=dev)
        t = (t[None] if t.ndim == 0 else t).to(torch.float32).expand(B).contiguous()
        ehs = encoder_hidden_states.to(device=dev, dtype=torch.bfloat16)
        if ehs.shape[0] not in (1, B):
            raise ValueError(f"encoder_hidden_states batch {ehs.shape[0]} for {B} videos")
        ehs = ehs.expand(B, -1, -1).contiguous()
        L = ehs.shape[1]
        ctx = self.make_ctx(ops.timestep_embed(t, self.time_proj.num_channels), ehs.reshape(B * L, -1), B, Fr, L)
        emb = self.embed_condition(self.condition_rows(controlnet_cond, conditioning_mask), B * Fr, ds * H, ds * W)
        res = self.forward_rows(emb, H, W, ctx)
        n = len(res)
        scales = [float(conditioning_scale) * s for s in (guess_mode_scales(n) if guess_mode else [1.0] * n)]
        if any(s != 1.0 for s in scales):
            sdev = torch.tensor(scales, dtype=torch.float32, device=dev)
            for i, a in enumerate(res):
                ops.scale_rows_(a.t, sdev[i:i + 1])
        maps = [rows_fmap(a.t, (a.n, a.c, a.h, a.w)) for a in res]
        if not return_dict:
            return tuple(maps[:-1]), maps[-1]
        return ControlNetOutput(tuple(maps[:-1]), maps[-1])


def sparse_controlnet_config_from_diffusers(cfg: dict) -> dict:
    """A diffusers SparseControlNetModel config.json -> this module's config; everything outside
    the SD-1.5 + AnimateDiff tree is refused by name."""
    if cfg.get("use_linear_projection"):
        raise NotImplementedError("use_linear_projection is not built: the transformer's proj_in / proj_out are "
                                  "1x1 convs here")
    if cfg.get("global_pool_conditions"):
        raise NotImplementedError("global_pool_conditions (pooled residuals) is not built")
    if cfg.get("controlnet_conditioning_channel_order", "rgb") != "rgb":
        raise NotImplementedError(f"controlnet_conditioning_channel_order="
                                  f"{cfg['controlnet_conditioning_channel_order']!r}: only 'rgb' is built")
    types = tuple(cfg.get("down_block_types", ("CrossAttnDownBlockMotion",) * 3 + ("DownBlockMotion",)))
    if any(t not in _DOWN_MOTION for t in types):
        raise NotImplementedError(f"down_block_types {types}: only {_DOWN_MOTION} are built")
    for k in ("transformer_layers_per_block", "temporal_transformer_layers_per_block",
              "transformer_layers_per_mid_block"):
        v = cfg.get(k, 1)
        if isinstance(v, (list, tuple)):
            if any(x != 1 for x in v):
                raise NotImplementedError(f"{k}={v!r}: one layer per block is built")
        elif v not in (1, None):
            raise NotImplementedError(f"{k}={v!r}: one layer per block is built")
    if cfg.get("only_cross_attention"):
        raise NotImplementedError("only_cross_attention is not built")
    if not cfg.get("concat_conditioning_mask", True):
        raise NotImplementedError("concat_conditioning_mask=False is not built: the condition rows always carry "
                                  "their mask column")
    lpb = cfg.get("layers_per_block", 2)
    if isinstance(lpb, (list, tuple)):
        raise NotImplementedError("per-block layers_per_block")
    heads = cfg.get("num_attention_heads") or cfg.get("attention_head_dim", 8)  # diffusers' legacy name
    if isinstance(heads, (list, tuple)):
        if len(set(heads)) != 1:
            raise NotImplementedError(f"per-block attention heads {heads}")
        heads = heads[0]
    mheads = cfg.get("motion_num_attention_heads", 8)
    if isinstance(mheads, (list, tuple)):
        if len(set(mheads)) != 1:
            raise NotImplementedError(f"per-block motion_num_attention_heads {mheads}")
        mheads = mheads[0]
    return dict(
        in_channels=cfg.get("in_channels", 4), sample_size=cfg.get("sample_size", 64),
        block_out_channels=tuple(cfg.get("block_out_channels", (320, 640, 1280, 1280))), layers_per_block=lpb,
        down_block_types=types, norm_num_groups=cfg.get("norm_num_groups", 32), norm_eps=cfg.get("norm_eps", 1e-5),
        cross_attention_dim=cfg.get("cross_attention_dim", 768), num_attention_heads=heads,
        motion_num_attention_heads=mheads, motion_max_seq_length=cfg.get("motion_max_seq_length", 32),
        conditioning_channels=cfg.get("conditioning_channels", 4),
        conditioning_embedding_out_channels=tuple(cfg.get("conditioning_embedding_out_channels", (16, 32, 96, 256))),
        concat_conditioning_mask=True,
        use_simplified_condition_embedding=bool(cfg.get("use_simplified_condition_embedding", True)))
