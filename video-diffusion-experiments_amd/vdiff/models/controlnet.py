"""ControlNetModel — diffusers:ControlNetModel for SD-1.5 on MI355X: the UNet's encoder half
without motion modules, a conditioning embedding in front and one 1x1 "zero" conv behind every
skip and the mid block.  State-dict names are diffusers' (`controlnet_cond_embedding.blocks.3`,
`controlnet_down_blocks.7`, `controlnet_mid_block`, ...), so a published SD-1.5 ControlNet
folder loads through `ControlNetModel.from_pretrained(local_dir)`.

Compute: the existing kernels.  ResnetBlock2D.run / Transformer2DModel.run / Downsample2D.run
are the UNet's; the conditioning embedding's eight 3x3 convs are vd_gemm implicit GEMMs with a
SiLU epilogue, its `+ embedding` the residual epilogue of conv_in, the zero convs plain GEMMs.
The residuals leave `forward_rows` UNscaled: in the denoising loop their scale is applied where
they are added to the UNet's skips (vd_rows_eltwise op 7, ops.ctrl_add_), read on the device by
the step index; `forward` (diffusers' calling convention) scales them with op 3.
"""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn as nn

from .. import ops
from ..config import down_block_plan, get_config
from .blocks import Ctx, ResnetBlock2D, Transformer2DModel
from .layers import Act, Conv2d, Downsample2D, TimestepEmbedding, Timesteps, bf, f32, fmap_rows, rows_fmap
from .unet_motion import CIN_PAD, FrozenDict

ControlNetOutput = namedtuple("ControlNetOutput", ["down_block_res_samples", "mid_block_res_sample"])

# what a ControlNet config adds to the UNet config it shares its encoder with
CONTROLNET_FULL = dict(conditioning_channels=3, conditioning_embedding_out_channels=(16, 32, 96, 256))
CONTROLNET_TINY = dict(conditioning_channels=3, conditioning_embedding_out_channels=(16, 32, 32, 64))
_EXTRA = {"full": CONTROLNET_FULL, "tiny": CONTROLNET_TINY}


def controlnet_config(name_or_cfg) -> dict:
    """The UNet config of that name (vdiff.config) plus the conditioning embedding's channels."""
    if isinstance(name_or_cfg, dict):
        cfg = get_config(name_or_cfg)
        for k, v in CONTROLNET_FULL.items():
            cfg.setdefault(k, v)
    else:
        cfg = get_config(name_or_cfg)
        cfg.update(_EXTRA[name_or_cfg])
    cfg["conditioning_embedding_out_channels"] = tuple(cfg["conditioning_embedding_out_channels"])
    for k in ("up_block_types", "out_channels", "motion_num_attention_heads", "motion_max_seq_length",
              "use_motion_mid_block"):
        cfg.pop(k, None)
    cfg["down_block_types"] = tuple(t.replace("Motion", "2D") for t in cfg["down_block_types"])
    return cfg


def guess_mode_scales(n: int) -> list:
    """diffusers' guess-mode weights of the n residuals, mid last: logspace(-1, 0, n)."""
    return torch.logspace(-1, 0, n).tolist()


def control_scale_table(n_steps: int, n_res: int, scale: float = 1.0, guess_mode: bool = False,
                        start: float = 0.0, end: float = 1.0) -> torch.Tensor:
    """The [n_steps][n_res] fp32 scales of a run, as diffusers' AnimateDiffControlNetPipeline forms
    them: step i keeps `scale * (1 - float(i / n < start or (i + 1) / n > end))`, times
    logspace(-1, 0, n_res) per residual in guess mode."""
    if isinstance(scale, (list, tuple)) or isinstance(start, (list, tuple)) or isinstance(end, (list, tuple)):
        raise NotImplementedError("per-ControlNet lists of scales / guidance windows (MultiControlNet) are not supported")
    if start >= end and not (start == end == 0.0):
        raise ValueError(f"control guidance start {start} cannot be larger or equal to control guidance end {end}")
    if start < 0.0 or end > 1.0:
        raise ValueError(f"control guidance start {start} / end {end} outside [0, 1]")
    keep = torch.tensor([1.0 - float(i / n_steps < start or (i + 1) / n_steps > end) for i in range(n_steps)],
                        dtype=torch.float32)
    per = torch.logspace(-1, 0, n_res) if guess_mode else torch.ones(n_res)
    return (float(scale) * keep)[:, None] * per[None, :].to(torch.float32)


class ControlNetConditioningEmbedding(nn.Module):
    """diffusers:ControlNetConditioningEmbedding: conv_in, pairs of (c -> c, c -> c' stride 2)
    convs, conv_out; SiLU after every conv but the last.  8x down in all."""

    def __init__(self, conditioning_embedding_channels: int, conditioning_channels: int = 3,
                 block_out_channels=(16, 32, 96, 256)):
        super().__init__()
        boc = tuple(block_out_channels)
        self.conv_in = Conv2d(conditioning_channels, boc[0], 3, padding=1)
        self.blocks = nn.ModuleList()
        for cin, cout in zip(boc[:-1], boc[1:]):
            self.blocks.append(Conv2d(cin, cin, 3, padding=1))
            self.blocks.append(Conv2d(cin, cout, 3, padding=1, stride=2))
        self.conv_out = Conv2d(boc[-1], conditioning_embedding_channels, 3, padding=1)

    def convs(self):
        return [self.conv_in, *self.blocks, self.conv_out]

    def run(self, rows, n_img, h, w):
        """Packed NHWC rows [n_img * h * w, 8] of the conditioning images -> [n_img * h/8 * w/8, C]."""
        convs = self.convs()
        for i, c in enumerate(convs):
            last = i == len(convs) - 1
            rows, h, w = ops.conv3x3(rows, n_img, h, w, c._w, stride=c.stride[0], bias=c._b,
                                     act=ops.ACT_NONE if last else ops.ACT_SILU)
        return rows

    def max_elements_per_image(self, h, w):
        """The largest activation of one h x w image over the layers (vd_gemm bounds M * ldc)."""
        best = h * w * CIN_PAD
        for c in self.convs():
            h, w = (h - 1) // c.stride[0] + 1, (w - 1) // c.stride[0] + 1
            best = max(best, h * w * c.out_channels)
        return best

    def forward(self, conditioning):
        """(N, 3, H, W) in [0, 1] -> the (N, C, H/8, W/8) embedding (module path)."""
        n, _, h, w = conditioning.shape
        rows = ops.pack_latents(conditioning.float()[:, :, None].contiguous(), dup=1, cpad=CIN_PAD)
        out = self.run(rows, n, h, w)
        return rows_fmap(out, (n, out.shape[1], h // 8, w // 8))


class CrossAttnDownBlock2D(nn.Module):
    """diffusers:CrossAttnDownBlock2D: CrossAttnDownBlockMotion without its motion modules."""

    def __init__(self, in_channels, out_channels, temb_channels, num_layers, heads, cross_dim, add_downsample,
                 groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_channels if i == 0 else out_channels, out_channels,
                                                    temb_channels, groups, eps) for i in range(num_layers)])
        if cross_dim is not None:
            self.attentions = nn.ModuleList([Transformer2DModel(heads, out_channels // heads, out_channels,
                                                                cross_dim, groups) for _ in range(num_layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(out_channels, out_channels)]) if add_downsample else None

    def run(self, x: Act, ctx: Ctx):
        outs = []
        attns = getattr(self, "attentions", None)
        for i, res in enumerate(self.resnets):
            x = res.run(x, ctx)
            if attns is not None:
                x = attns[i].run(x, ctx)
            outs.append(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0].run(x)
            outs.append(x)
        return x, outs

    def forward(self, hidden_states, temb=None, encoder_hidden_states=None, **unused):
        outs = ()
        attns = getattr(self, "attentions", None)
        h = hidden_states
        for i, res in enumerate(self.resnets):
            h = res(h, temb)
            if attns is not None:
                h = attns[i](h, encoder_hidden_states=encoder_hidden_states, return_dict=False)[0]
            outs = outs + (h,)
        if self.downsamplers is not None:
            for d in self.downsamplers:
                h = d(h)
            outs = outs + (h,)
        return h, outs


class DownBlock2D(CrossAttnDownBlock2D):
    """diffusers:DownBlock2D (no attentions)."""

    def __init__(self, in_channels, out_channels, temb_channels, num_layers, add_downsample, groups, eps):
        super().__init__(in_channels, out_channels, temb_channels, num_layers, None, None, add_downsample, groups, eps)


class UNetMidBlock2DCrossAttn(nn.Module):
    """diffusers:UNetMidBlock2DCrossAttn: resnet, transformer, resnet."""

    def __init__(self, channels, temb_channels, heads, cross_dim, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(channels, channels, temb_channels, groups, eps) for _ in range(2)])
        self.attentions = nn.ModuleList([Transformer2DModel(heads, channels // heads, channels, cross_dim, groups)])

    def run(self, x: Act, ctx: Ctx) -> Act:
        x = self.resnets[0].run(x, ctx)
        x = self.attentions[0].run(x, ctx)
        return self.resnets[1].run(x, ctx)

    def forward(self, hidden_states, temb=None, encoder_hidden_states=None, **unused):
        h = self.resnets[0](hidden_states, temb)
        h = self.attentions[0](h, encoder_hidden_states=encoder_hidden_states, return_dict=False)[0]
        return self.resnets[1](h, temb)


class ControlNetModel(nn.Module):
    def __init__(self, config="full"):
        super().__init__()
        cfg = controlnet_config(config)
        self.config = FrozenDict(cfg)
        boc = cfg["block_out_channels"]
        g, eps = cfg["norm_num_groups"], cfg["norm_eps"]
        heads, cross = cfg["num_attention_heads"], cfg["cross_attention_dim"]
        tdim = boc[0] * 4
        self.conv_in = Conv2d(cfg["in_channels"], boc[0], 3, padding=1)
        self.time_proj = Timesteps(boc[0])
        self.time_embedding = TimestepEmbedding(boc[0], tdim)
        self.controlnet_cond_embedding = ControlNetConditioningEmbedding(
            boc[0], cfg["conditioning_channels"], cfg["conditioning_embedding_out_channels"])
        self.down_blocks = nn.ModuleList()
        self.controlnet_down_blocks = nn.ModuleList([Conv2d(boc[0], boc[0], 1)])
        for (out_ch, ins, has_attn, down) in down_block_plan(cfg):
            if has_attn:
                blk = CrossAttnDownBlock2D(ins[0], out_ch, tdim, len(ins), heads, cross, down, g, eps)
            else:
                blk = DownBlock2D(ins[0], out_ch, tdim, len(ins), down, g, eps)
            self.down_blocks.append(blk)
            for _ in range(len(ins) + int(down)):
                self.controlnet_down_blocks.append(Conv2d(out_ch, out_ch, 1))
        self.controlnet_mid_block = Conv2d(boc[-1], boc[-1], 1)
        self.mid_block = UNetMidBlock2DCrossAttn(boc[-1], tdim, heads, cross, g, eps)
        self._prepared = False

    # ------------------------------------------------------------------ utils
    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def num_residuals(self) -> int:
        """Down residuals plus the mid one: 13 for SD-1.5, 5 for the tiny config."""
        return len(self.controlnet_down_blocks) + 1

    def residual_channels(self) -> list:
        return [c.out_channels for c in self.controlnet_down_blocks] + [self.controlnet_mid_block.out_channels]

    def resnets_in_order(self):
        return [m for m in self.modules() if isinstance(m, ResnetBlock2D)]

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=None, variant=None, device="cuda", **unused):
        """diffusers ControlNetModel.from_pretrained over a LOCAL folder (config.json +
        diffusion_pytorch_model[.variant].safetensors), bf16 on `device`."""
        from .. import pretrained as P
        if isinstance(pretrained_model_name_or_path, (list, tuple)):
            raise NotImplementedError("a list of ControlNets (MultiControlNetModel) is not supported: load one")
        d = P._local_dir(pretrained_model_name_or_path, "ControlNetModel.from_pretrained")
        cfg = controlnet_config_from_diffusers(P.read_json(d / "config.json"))
        m = P._assign(P._empty_on(cls, cfg, device), P.load_weights(d, variant), what="ControlNetModel")
        m.torch_dtype = torch_dtype
        return m

    @torch.no_grad()
    def prepare(self):
        """Pack device operands for the HIP kernels (idempotent; re-run after a weight load)."""
        if not next(self.parameters()).is_cuda:
            raise RuntimeError("ControlNetModel.prepare(): move the model to the GPU first (no CPU path)")
        for m in self.modules():
            if m is not self and hasattr(m, "prepare"):
                m.prepare()
        assert self.conv_in._cin_pad == CIN_PAD and self.controlnet_cond_embedding.conv_in._cin_pad == CIN_PAD
        res = self.resnets_in_order()
        off = 0
        for r in res:  # the ControlNet's own offsets into its own concatenated time_emb_proj table
            r.temb_offset = off
            off += r.out_channels
        self._w_temb = bf(torch.cat([r.time_emb_proj.weight for r in res], 0))
        self._b_temb = f32(torch.cat([r.time_emb_proj.bias for r in res], 0))
        self._prepared = True
        return self

    # ------------------------------------------------------------------ core
    def make_ctx(self, t_emb_bf16, ehs_rows, batch, frames, ctx_len, kv_cache=None):
        temb_silu = self.time_embedding.forward_silu(t_emb_bf16)
        temb_all = ops.gemm(temb_silu, self._w_temb, bias=self._b_temb, out_f32=True)
        return Ctx(batch, frames, temb_all, ehs_rows, ctx_len, kv_cache=kv_cache, ip_rows=None)

    @torch.no_grad()
    def embed_condition(self, cond):
        """(B, 3, F, 8h, 8w) fp32 in [0, 1] -> the embedding's bf16 NHWC rows [B * F * h * w, C0].
        It depends on no timestep: the pipeline computes it once per video.  Frames are chunked
        where one launch's activation would pass vd_gemm's 2^31-element bound."""
        if not self._prepared:
            self.prepare()
        if cond.dim() != 5 or cond.shape[1] != self.config["conditioning_channels"]:
            raise ValueError(f"controlnet_cond: expected (B, {self.config['conditioning_channels']}, F, H, W), "
                             f"got {tuple(cond.shape)}")
        B, _, Fr, H, W = cond.shape
        if H % 8 or W % 8:
            raise ValueError(f"conditioning frames must be multiples of 8 in height and width, got {H} x {W}")
        emb = self.controlnet_cond_embedding
        cond = cond.to(self.device, torch.float32)
        per = emb.max_elements_per_image(H, W)
        if per >= 0x7fffffff:
            raise ValueError(f"one {H} x {W} conditioning frame exceeds the conv kernels' 2^31-element bound")
        chunk = max(1, (0x7fffffff - 1) // per)
        hw = (H // 8) * (W // 8)
        out = torch.empty(B * Fr * hw, emb.conv_out.out_channels, device=self.device, dtype=torch.bfloat16)
        for b in range(B):
            for f0 in range(0, Fr, chunk):
                n = min(chunk, Fr - f0)
                rows = ops.pack_latents(cond[b:b + 1, :, f0:f0 + n].contiguous(), dup=1, cpad=CIN_PAD)
                out[(b * Fr + f0) * hw:(b * Fr + f0 + n) * hw].copy_(emb.run(rows, n, H, W))
        return out

    def forward_rows(self, x_rows, cond_rows, h, w, ctx: Ctx):
        """Packed NHWC input rows [batch*frames*h*w, 8] and embed_condition's rows of the same
        images -> the UNscaled zero-conv outputs as Acts: one per UNet skip, then the mid one."""
        n_img = ctx.batch * ctx.frames
        if cond_rows.shape[0] != x_rows.shape[0]:
            raise ValueError(f"{cond_rows.shape[0]} conditioning rows for {x_rows.shape[0]} latent rows")
        t, _, _ = ops.conv3x3(x_rows, n_img, h, w, self.conv_in._w, bias=self.conv_in._b, res=cond_rows)
        x = Act(t, n_img, h, w)
        outs = [x]
        for blk in self.down_blocks:
            x, o = blk.run(x, ctx)
            outs.extend(o)
        outs.append(self.mid_block.run(x, ctx))
        zero = [*self.controlnet_down_blocks, self.controlnet_mid_block]
        return [Act(ops.gemm(a.t, z._w, bias=z._b), a.n, a.h, a.w) for a, z in zip(outs, zero)]

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0,
                class_labels=None, timestep_cond=None, attention_mask=None, added_cond_kwargs=None,
                cross_attention_kwargs=None, guess_mode: bool = False, return_dict: bool = True):
        """diffusers ControlNetModel.forward: sample (N, C, H, W) with N = batch * frames,
        encoder_hidden_states (N, L, D) or (1, L, D), controlnet_cond (N, 3, 8H, 8W) in [0, 1]
        -> ControlNetOutput of (N, C_i, H_i, W_i) bf16 residuals times conditioning_scale (times
        logspace(-1, 0, n) in guess mode)."""
        if not self._prepared:
            self.prepare()
        for unsupported, name in ((class_labels, "class_labels"), (timestep_cond, "timestep_cond"),
                                  (attention_mask, "attention_mask"), (added_cond_kwargs, "added_cond_kwargs")):
            if unsupported is not None:
                raise NotImplementedError(f"{name} is not supported by this ControlNetModel")
        if isinstance(conditioning_scale, (list, tuple)):
            raise NotImplementedError("a list of conditioning scales (MultiControlNetModel) is not supported")
        if sample.dim() != 4:
            raise ValueError(f"sample: expected (batch*frames, C, H, W), got {tuple(sample.shape)}")
        dev = self.device
        N, _, H, W = sample.shape
        if controlnet_cond.dim() != 4 or controlnet_cond.shape[0] != N or \
                tuple(controlnet_cond.shape[2:]) != (8 * H, 8 * W):
            raise ValueError(f"controlnet_cond of shape {tuple(controlnet_cond.shape)}: expected ({N}, "
                             f"{self.config['conditioning_channels']}, {8 * H}, {8 * W})")
        t = torch.as_tensor(timestep, device=dev)
        t = (t[None] if t.ndim == 0 else t).to(torch.float32).expand(N).contiguous()
        ehs = encoder_hidden_states.to(device=dev, dtype=torch.bfloat16)
        if ehs.shape[0] not in (1, N):
            raise ValueError(f"encoder_hidden_states batch {ehs.shape[0]} for {N} images")
        ehs = ehs.expand(N, -1, -1).contiguous()
        L = ehs.shape[1]
        # every image is its own "video" of one frame: its own timestep row and text rows
        ctx = self.make_ctx(ops.timestep_embed(t, self.time_proj.num_channels), ehs.reshape(N * L, -1), N, 1, L)
        cond_rows = self.embed_condition(controlnet_cond.to(dev).float().permute(1, 0, 2, 3)[None].contiguous())
        x_rows = ops.pack_latents(sample.to(dev).float()[:, :, None].contiguous(), dup=1, cpad=CIN_PAD)
        res = self.forward_rows(x_rows, cond_rows, H, W, ctx)
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


_DOWN_2D = ("CrossAttnDownBlock2D", "DownBlock2D")


def controlnet_config_from_diffusers(cfg: dict) -> dict:
    """A diffusers ControlNetModel config.json -> this module's config; everything outside the
    SD-1.5 tree is refused by name."""
    if cfg.get("use_linear_projection"):
        raise NotImplementedError("use_linear_projection (SD-2.x ControlNets) is not built: the transformer's "
                                  "proj_in / proj_out are 1x1 convs here")
    for k in ("class_embed_type", "num_class_embeds", "addition_embed_type", "projection_class_embeddings_input_dim",
              "addition_time_embed_dim", "encoder_hid_dim", "encoder_hid_dim_type"):
        if cfg.get(k) is not None:
            raise NotImplementedError(f"{k}={cfg[k]!r}: class / addition embeddings (SDXL ControlNets) are not built")
    if cfg.get("global_pool_conditions"):
        raise NotImplementedError("global_pool_conditions (the shuffle ControlNet's pooled residuals) is not built")
    if cfg.get("controlnet_conditioning_channel_order", "rgb") != "rgb":
        raise NotImplementedError(f"controlnet_conditioning_channel_order="
                                  f"{cfg['controlnet_conditioning_channel_order']!r}: only 'rgb' is built")
    types = tuple(cfg.get("down_block_types", ("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",)))
    if any(t not in _DOWN_2D for t in types):
        raise NotImplementedError(f"down_block_types {types}: only {_DOWN_2D} are built")
    if cfg.get("mid_block_type", "UNetMidBlock2DCrossAttn") != "UNetMidBlock2DCrossAttn":
        raise NotImplementedError(f"mid_block_type {cfg['mid_block_type']!r}")
    if cfg.get("transformer_layers_per_block", 1) != 1 or cfg.get("only_cross_attention"):
        raise NotImplementedError("transformer_layers_per_block != 1 / only_cross_attention are not built")
    lpb = cfg.get("layers_per_block", 2)
    if isinstance(lpb, (list, tuple)):
        raise NotImplementedError("per-block layers_per_block")
    heads = cfg.get("num_attention_heads") or cfg.get("attention_head_dim", 8)  # diffusers' legacy name
    if isinstance(heads, (list, tuple)):
        if len(set(heads)) != 1:
            raise NotImplementedError(f"per-block attention heads {heads}")
        heads = heads[0]
    return dict(
        in_channels=cfg.get("in_channels", 4), sample_size=cfg.get("sample_size", 64),
        block_out_channels=tuple(cfg.get("block_out_channels", (320, 640, 1280, 1280))), layers_per_block=lpb,
        down_block_types=types, norm_num_groups=cfg.get("norm_num_groups", 32), norm_eps=cfg.get("norm_eps", 1e-5),
        cross_attention_dim=cfg.get("cross_attention_dim", 768), num_attention_heads=heads,
        conditioning_channels=cfg.get("conditioning_channels", 3),
        conditioning_embedding_out_channels=tuple(cfg.get("conditioning_embedding_out_channels", (16, 32, 96, 256))))
