"""UNetMotionModel — drop-in for diffusers:UNetMotionModel (SD-1.5 +
animatediff-motion-adapter) on MI355X.

Call surface kept from the reference's use (experiments/03_trace_forward_pass.py:
86-115): `unet(sample[B,C,F,H,W], timestep, encoder_hidden_states=
[B,L,D]).sample`, `.config`, `.dtype`, `.device`, and the diffusers module tree
(`down_blocks[i].{resnets,attentions,motion_modules,downsamplers}`, `mid_block`,
`up_blocks`, class `Attention` with `.heads`/`.to_q.in_features`).

Compute: every op runs in libvdiff_hip.so (bf16 activations, fp32
accumulation/statistics, fp32 output).  Call `prepare()` once after moving the
model to the GPU (done lazily by forward).
"""
from __future__ import annotations

import re
from collections import namedtuple
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..config import down_block_plan, get_config, up_block_plan
from .blocks import (FREE_NOISE_WEIGHTING_SCHEMES, AnimateDiffTransformer3D, CrossAttnDownBlockMotion,
                     CrossAttnUpBlockMotion, Ctx, DownBlockMotion, ResnetBlock2D, UNetMidBlockCrossAttnMotion,
                     UpBlockMotion)
from .layers import (Act, Attention, Conv2d, GroupNorm, SiLU, TimestepEmbedding, Timesteps, add, bf, f32, fmap_rows, rows_fmap,
                     token_rows)


class FrozenDict(dict):
    """diffusers-style config: dict + attribute access."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


UNetMotionOutput = namedtuple("UNetMotionOutput", ["sample"])


def fmap_rows_f32(x):
    """fp32 channels-last (N, C, H, W) -> its NHWC rows (conv_out's output)."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])

CIN_PAD = 8  # conv_in input channels padded 4 -> 8 (16-byte NHWC rows)


def pag_layer_matches(layer_id: str, name: str) -> bool:
    """diffusers' PAGMixin._set_pag_attn_processor rule for one self-attention module name: the
    layer id is a regular expression applied with re.search, and an id that ends in digits must
    not be followed by another digit ("down_blocks.1" does not select "down_blocks.10...")."""
    pattern = f"(?:{layer_id})(?![0-9])" if layer_id[-1:].isdigit() else layer_id
    return re.search(pattern, name) is not None


def pag_select(layers, self_attn_names):
    """The self-attention names `layers` (a layer id or a list of them) select, in module order.
    A layer id that selects none raises ValueError naming it."""
    layers = [layers] if isinstance(layers, str) else list(layers)
    names = list(self_attn_names)
    picked = set()
    for layer_id in layers:
        if not isinstance(layer_id, str) or not layer_id:
            raise ValueError(f"pag_applied_layers holds {layer_id!r}: each entry is a non-empty string")
        hit = [n for n in names if pag_layer_matches(layer_id, n)]
        if not hit:
            raise ValueError(f"Cannot find PAG layer to set attention processor for: {layer_id}")
        picked.update(hit)
    return [n for n in names if n in picked]


class ControlResiduals:
    """ControlNet residuals given to UNetMotionModel.forward, as bf16 NHWC rows: added as they
    are (their scale is already in them) with ops.rows_add, in place."""

    def __init__(self, down_rows, mid_rows):
        self.down_rows, self.mid_rows = list(down_rows), mid_rows

    def inject(self, skips, mid, ctx):
        for s, r in zip(skips, self.down_rows):
            ops.rows_add(s.t, r, out=s.t)
        ops.rows_add(mid.t, self.mid_rows, out=mid.t)


class UNetMotionModel(nn.Module):
    def __init__(self, config="full"):
        super().__init__()
        cfg = get_config(config)
        self.config = FrozenDict(cfg)
        boc = cfg["block_out_channels"]
        g, eps = cfg["norm_num_groups"], cfg["norm_eps"]
        heads, mheads = cfg["num_attention_heads"], cfg["motion_num_attention_heads"]
        cross, mlen = cfg["cross_attention_dim"], cfg["motion_max_seq_length"]
        tdim = boc[0] * 4
        self.conv_in = Conv2d(cfg["in_channels"], boc[0], 3, padding=1)
        self.time_proj = Timesteps(boc[0])
        self.time_embedding = TimestepEmbedding(boc[0], tdim)
        self.down_blocks = nn.ModuleList()
        for (out_ch, ins, has_attn, down) in down_block_plan(cfg):
            if has_attn:
                blk = CrossAttnDownBlockMotion(ins[0], out_ch, tdim, len(ins), heads, cross, mheads, down,
                                               g, eps, mlen)
            else:
                blk = DownBlockMotion(ins[0], out_ch, tdim, len(ins), mheads, down, g, eps, mlen)
            self.down_blocks.append(blk)
        self.up_blocks = nn.ModuleList()
        for (out_ch, ins, has_attn, up) in up_block_plan(cfg):
            if has_attn:
                blk = CrossAttnUpBlockMotion(ins, out_ch, tdim, heads, cross, mheads, up, g, eps, mlen)
            else:
                blk = UpBlockMotion(ins, out_ch, tdim, mheads, up, g, eps, mlen)
            blk.resolution_idx = len(self.up_blocks)
            self.up_blocks.append(blk)
        self.mid_block = UNetMidBlockCrossAttnMotion(boc[-1], tdim, heads, cross, mheads, g, eps, mlen,
                                                     use_motion=cfg.get("use_motion_mid_block", True))
        self.conv_norm_out = GroupNorm(g, boc[0], eps=eps)
        self.conv_act = SiLU()
        self.conv_out = Conv2d(boc[0], cfg["out_channels"], 3, padding=1)
        self.conv_out.out_f32 = True  # eps leaves the UNet in fp32
        self._prepared = False
        self.dist = None  # vdiff.dist.FrameShard when frames are sharded across ranks

    # ------------------------------------------------------------------ utils
    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def device(self):
        return next(self.parameters()).device

    def resnets_in_order(self):
        return [m for m in self.modules() if isinstance(m, ResnetBlock2D)]

    @torch.no_grad()
    def prepare(self):
        """Pack device operands for the HIP kernels (idempotent; re-run after a weight load)."""
        if not next(self.parameters()).is_cuda:
            raise RuntimeError("UNetMotionModel.prepare(): move the model to the GPU first (no CPU path)")
        for m in self.modules():
            if m is not self and hasattr(m, "prepare"):
                m.prepare()  # every module packs only its own operands
        assert self.conv_in._cin_pad == CIN_PAD
        res = self.resnets_in_order()
        off = 0
        for r in res:
            r.temb_offset = off
            off += r.out_channels
        self._w_temb = bf(torch.cat([r.time_emb_proj.weight for r in res], 0))
        self._b_temb = f32(torch.cat([r.time_emb_proj.bias for r in res], 0))
        self._prepared = True
        return self

    # ------------------------------------------------------------------ core
    def make_ctx(self, t_emb_bf16, ehs_rows, batch, frames, ctx_len, kv_cache=None, ip_rows=None, pag_batch=0):
        temb_silu = self.time_embedding.forward_silu(t_emb_bf16)
        temb_all = ops.gemm(temb_silu, self._w_temb, bias=self._b_temb, out_f32=True)
        ctx = Ctx(batch, frames, temb_all, ehs_rows, ctx_len, dist=self.dist, kv_cache=kv_cache, ip_rows=ip_rows)
        ctx.pag_batch = pag_batch
        return ctx

    # ------------------------------------------------------------------ IP-Adapter
    def spatial_cross_attentions(self):
        """The non-motion cross-attentions (attn2 of every spatial transformer block) in the
        order an IP-Adapter checkpoint numbers them: down_blocks, up_blocks, mid_block
        (vdiff.pretrained.IP_ADAPTER_BLOCK_ORDER)."""
        from ..pretrained import IP_ADAPTER_BLOCK_ORDER
        out = []
        for name in IP_ADAPTER_BLOCK_ORDER:
            blks = getattr(self, name)
            for blk in (blks if isinstance(blks, nn.ModuleList) else [blks]):
                for tm in getattr(blk, "attentions", None) or []:
                    out.extend(tb.attn2 for tb in tm.transformer_blocks)
        return out

    @property
    def has_ip_adapter(self) -> bool:
        return any("to_k_ip" in a._modules for a in self.spatial_cross_attentions())

    @torch.no_grad()
    def set_ip_adapter_weights(self, kv_weights, scale: float = 1.0):
        """kv_weights: one (to_k_ip.weight, to_v_ip.weight) pair per spatial cross-attention, in
        spatial_cross_attentions() order."""
        attns = self.spatial_cross_attentions()
        if len(kv_weights) != len(attns):
            raise ValueError(f"{len(kv_weights)} to_k_ip / to_v_ip pairs for {len(attns)} cross-attentions")
        for a, (wk, wv) in zip(attns, kv_weights):
            a.add_ip_adapter(wk, wv)
        self.set_ip_adapter_scale(scale)

    @torch.no_grad()
    def set_ip_adapter_scale(self, scale: float):
        """Re-packs only the [to_k_ip ; s * to_v_ip] operands (the scale lives in the V rows)."""
        if not isinstance(scale, (int, float)):
            raise NotImplementedError("per-block IP-Adapter scales (a dict or list) are not supported: one float")
        for a in self.spatial_cross_attentions():
            a.ip_scale = float(scale)
            if self._prepared:
                a.prepare_ip()

    def unload_ip_adapter(self):
        for a in self.spatial_cross_attentions():
            a.remove_ip_adapter()

    # ------------------------------------------------------------------ LoRA
    def load_lora_state_dict(self, state_dict, adapter_name=None, weight: float = 1.0):
        """Merge a LoRA (any key layout of vdiff.lora) into the parameters as a new active adapter
        and re-pack the operands; -> the adapter's name.  A DenoiseLoop built before keeps the
        operands it was built with: load and set adapters before the pipeline call."""
        from .. import lora
        return lora.load_lora_state_dict(self, state_dict, adapter_name=adapter_name, weight=weight)

    def set_adapters(self, adapter_names, weights=None):
        from .. import lora
        lora.set_adapters(self, adapter_names, weights)

    def get_active_adapters(self):
        from .. import lora
        return lora.get_active_adapters(self)

    def delete_adapters(self, adapter_names):
        from .. import lora
        lora.delete_adapters(self, adapter_names)

    def unload_lora(self):
        """Every parameter back to its base tensor, bit for bit."""
        from .. import lora
        lora.unload(self)

    # ------------------------------------------------------------------ perturbed-attention guidance
    def self_attention_names(self):
        """The diffusers module names of every self-attention: attn1 of the spatial transformer
        blocks, attn1 and attn2 of the motion modules' (cross-attentions are never perturbed)."""
        return [n for n, m in self.named_modules() if isinstance(m, Attention) and not m.is_cross]

    def set_pag_applied_layers(self, layers):
        """Mark the self-attentions PAG perturbs (diffusers' PAGMixin.set_pag_applied_layers +
        _set_pag_attn_processor; pag_select has the matching rule) and return their names.  None or
        an empty list clears the marks.  A marked attention runs the perturbed videos of a batch
        (Ctx.pag_batch, set by DenoiseLoop(pag=...)) through to_v and to_out alone; everything else,
        the hooked module path included, is unchanged."""
        names = pag_select(layers, self.self_attention_names()) if layers else []
        chosen = set(names)
        for n, m in self.named_modules():
            if isinstance(m, Attention):
                m.pag = n in chosen
        return names

    def pag_applied_layers(self):
        return [n for n, m in self.named_modules() if isinstance(m, Attention) and m.pag]

    # ------------------------------------------------------------------ FreeU
    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers' FreeUMixin.enable_freeu: s1 / b1 act in up_blocks[0], s2 / b2 in
        up_blocks[1] — before each skip concat the skip's four lowest frequency bins are scaled by
        s and the first half of the backbone channels by b (vd_rows_eltwise ops 2 and 3).  The
        attributes are set on every up block, as diffusers does; a DenoiseLoop built afterwards
        captures the extra launches, one built before keeps running without them."""
        for blk in self.up_blocks:
            blk.s1, blk.s2, blk.b1, blk.b2 = s1, s2, b1, b2
            blk.prepare()

    def disable_freeu(self):
        for blk in self.up_blocks:
            blk.s1 = blk.s2 = blk.b1 = blk.b2 = None
            blk.prepare()

    # ------------------------------------------------------------------ FreeNoise
    def motion_modules_in_order(self):
        return [m for m in self.modules() if isinstance(m, AnimateDiffTransformer3D)]

    def enable_free_noise(self, context_length=16, context_stride=4, weighting_scheme="pyramid"):
        """diffusers' AnimateDiffFreeNoiseMixin on the UNet: every motion module runs its
        transformer block on sliding windows of context_length frames, context_stride apart, and
        averages the window outputs with the scheme's per-frame weights (vd_rows_eltwise ops 4
        and 5 around the unchanged temporal kernels), so a video may be longer than
        motion_max_seq_length.  context_length None is motion_max_seq_length.  A call with
        exactly context_length frames runs as without FreeNoise, one with fewer raises.  A
        DenoiseLoop built afterwards captures the windowed launches, one built before keeps
        running without them."""
        mlen = self.config["motion_max_seq_length"]
        L = mlen if context_length is None else context_length
        if not isinstance(L, int) or not isinstance(context_stride, int) or isinstance(L, bool):
            raise ValueError(f"context_length and context_stride must be integers, got {L!r}, {context_stride!r}")
        if L < 1 or L > mlen:
            raise ValueError(f"context_length {L} is outside 1..motion_max_seq_length={mlen}: the positional "
                             "table and the temporal kernels end there")
        if not 1 <= context_stride <= L:
            raise ValueError(f"context_stride {context_stride} is outside 1..context_length={L}")
        if weighting_scheme not in FREE_NOISE_WEIGHTING_SCHEMES:
            raise ValueError(f"weighting_scheme {weighting_scheme!r}: one of {FREE_NOISE_WEIGHTING_SCHEMES}")
        for m in self.motion_modules_in_order():
            m.context_length, m.context_stride, m.weighting_scheme = L, context_stride, weighting_scheme
            m.prepare()

    def disable_free_noise(self):
        for m in self.motion_modules_in_order():
            m.context_length = m.context_stride = m.weighting_scheme = None
            m.prepare()

    @property
    def free_noise_enabled(self) -> bool:
        return any(m.free_noise_enabled for m in self.motion_modules_in_order())

    def control_residual_shapes(self, n_img, h, w):
        """(rows, channels) of every down-block skip, in order, then of the mid block's output:
        what down_block_additional_residuals / mid_block_additional_residual must match."""
        shapes = [(n_img * h * w, self.conv_in.out_channels)]
        for blk in self.down_blocks:
            c = blk.resnets[0].out_channels
            shapes += [(n_img * h * w, c)] * len(blk.resnets)
            if blk.downsamplers is not None:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                shapes.append((n_img * h * w, c))
        return shapes + [(n_img * h * w, self.mid_block.resnets[-1].out_channels)]

    def _control_residuals(self, down, mid, n_img, H, W):
        """The two residual arguments of forward -> ControlResiduals, or None when neither is given."""
        if down is None and mid is None:
            return None
        if down is None or mid is None:
            raise ValueError("down_block_additional_residuals and mid_block_additional_residual go together "
                             "(a ControlNet returns both)")
        shapes = self.control_residual_shapes(n_img, H, W)
        maps = list(down) + [mid]
        if len(maps) != len(shapes):
            raise ValueError(f"{len(maps) - 1} down-block residuals for this UNet's {len(shapes) - 1} skips")
        for i, (m, (r, c)) in enumerate(zip(maps, shapes)):
            if m.dim() != 4 or m.shape[0] != n_img or m.shape[1] != c or m.shape[0] * m.shape[2] * m.shape[3] != r:
                raise ValueError(f"control residual {i} of shape {tuple(m.shape)}: expected ({n_img}, {c}, h, w) "
                                 f"with {r // n_img} pixels")
        rows = [fmap_rows(m.to(self.device)) for m in maps]
        return ControlResiduals(rows[:-1], rows[-1])

    def forward_rows(self, x_rows, h, w, ctx: Ctx, control=None):
        """Packed NHWC input rows [batch*frames*h*w, 8] -> eps rows fp32 [..., out_channels].
        control: an object whose inject(skips, mid, ctx) adds ControlNet residuals in place
        (ControlResiduals, or the denoising loop's vdiff.pipeline.ControlState).  It runs after
        the mid block: the last skip is also the mid block's input and must not change earlier."""
        g = self.config["norm_num_groups"]
        n_img = ctx.batch * ctx.frames
        blocks = list(self.down_blocks)
        res0 = None
        if ctx.cfg_dup and ctx.batch % 2 == 0:
            # CFG dedup: both halves of x_rows are the same latents and the same timestep, so
            # conv_in, down_blocks[0].resnets[0] and attentions[0] up to its cross-attention
            # (nothing reads the text embeddings before it) run on one half; their outputs are
            # copied to the other
            # (planned as the whole batch, ops.plan_scaled: the same kernels, the same bits)
            half = x_rows.shape[0] // 2
            t = torch.empty(x_rows.shape[0], self.conv_in.out_channels, device=x_rows.device, dtype=torch.bfloat16)
            with ops.plan_scaled(2):
                ops.conv3x3(x_rows[:half], n_img // 2, h, w, self.conv_in._w, bias=self.conv_in._b, out=t[:half])
                r1 = blocks[0].resnets[0].run(Act(t[:half], n_img // 2, h, w), ctx)
            t[half:].copy_(t[:half])
            res0 = (Act(None, n_img, h, w), r1)  # the full batch is never materialised
        else:
            t, _, _ = ops.conv3x3(x_rows, n_img, h, w, self.conv_in._w, bias=self.conv_in._b)
        x = Act(t, n_img, h, w)
        skips = [x]
        for i, blk in enumerate(blocks):
            x, outs = blk.run(x, ctx, res0=res0) if i == 0 else blk.run(x, ctx)
            skips.extend(outs)
        x = self.mid_block.run(x, ctx)
        if control is not None:
            control.inject(skips, x, ctx)
        for blk in self.up_blocks:
            x = blk.run(x, ctx, skips)
        no = self.conv_norm_out
        hn = ops.group_norm(x.t, x.n, x.h * x.w, g, self.config["norm_eps"], no._g, no._b, silu=True)
        eps, _, _ = ops.conv3x3(hn, x.n, x.h, x.w, self.conv_out._w, bias=self.conv_out._b, out_f32=True)
        return eps

    def has_hooks(self) -> bool:
        """Forward (pre-)hooks registered on any module of the tree, or globally."""
        from torch.nn.modules import module as _m
        if _m._global_forward_hooks or _m._global_forward_pre_hooks:
            return True
        return any(m._forward_hooks or m._forward_pre_hooks for m in self.modules() if m is not self)

    def forward_modules(self, sample, t, ehs, control=None):
        """diffusers UNetMotionModel.forward module by module: every block
        and leaf through __call__ with diffusers-layout tensors, all on the HIP kernels — the
        path a forward-hook trace (experiments/03_trace_forward_pass.py:105-113) observes.
        Unsharded only: its motion modules attend over the frames they are given, so under a
        FrameShard they would see the rank's local frames alone."""
        if getattr(self, "dist", None) is not None:
            raise NotImplementedError("forward hooks are not supported under frame sharding "
                                      "(UNetMotionModel.dist is set): the module path has no "
                                      "cross-rank temporal window; detach the hooks or the FrameShard")
        B, Cc, Fr, H, W = sample.shape
        L = ehs.shape[1]
        emb = self.time_embedding(self.time_proj(t))                       # (B, 1280)
        emb = ops.rows_add(None, emb, y_div=Fr, out=torch.empty(B * Fr, emb.shape[1], device=emb.device,
                                                                dtype=torch.bfloat16))  # repeat_interleave(F)
        if ehs.shape[0] == B * Fr:  # per-frame text (or one frame): the rows are (video, frame) already
            ehs_rep = ehs
        else:
            ehs_rows = token_rows(ehs)
            ehs_rep = torch.empty(B * Fr * L, ehs.shape[2], device=ehs.device, dtype=torch.bfloat16)
            for b in range(B):  # ehs.repeat_interleave(F, 0)
                ops.rows_add(None, ehs_rows[b * L:(b + 1) * L], out=ehs_rep[b * Fr * L:(b + 1) * Fr * L])
            ehs_rep = ehs_rep.view(B * Fr, L, -1)
        x = sample.permute(0, 2, 1, 3, 4).reshape(B * Fr, Cc, H, W)
        h = self.conv_in(x)
        skips = (h,)
        for blk in self.down_blocks:
            if isinstance(blk, DownBlockMotion):
                h, res = blk(h, emb, num_frames=Fr)
            else:
                h, res = blk(h, emb, encoder_hidden_states=ehs_rep, num_frames=Fr)
            skips = skips + res
        h = self.mid_block(h, emb, encoder_hidden_states=ehs_rep, num_frames=Fr)
        if control is not None:  # diffusers: new skips = skip + residual, mid output + residual
            skips = tuple(add(sk, rows_fmap(r, tuple(sk.shape))) for sk, r in zip(skips, control.down_rows))
            h = add(h, rows_fmap(control.mid_rows, tuple(h.shape)))
        for blk in self.up_blocks:
            n = len(blk.resnets)
            res, skips = skips[-n:], skips[:-n]
            if isinstance(blk, UpBlockMotion):
                h = blk(h, res, emb, num_frames=Fr)
            else:
                h = blk(h, res, emb, encoder_hidden_states=ehs_rep, num_frames=Fr)
        h = self.conv_out(self.conv_act(self.conv_norm_out(h)))            # fp32 (B*F, C, H, W)
        return ops.unpack_nhwc(fmap_rows_f32(h), B, h.shape[1], Fr, H, W)

    def forward(self, sample, timestep, encoder_hidden_states, timestep_cond=None, attention_mask=None,
                cross_attention_kwargs=None, added_cond_kwargs=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None,
                return_dict: bool = True, num_frames: Optional[int] = None):
        if not self._prepared:
            self.prepare()
        for unsupported, name in ((timestep_cond, "timestep_cond"), (attention_mask, "attention_mask")):
            if unsupported is not None:
                raise NotImplementedError(f"{name} is not used by the reference's pipeline")
        dev = self.device
        B, Cc, Fr, H, W = sample.shape
        t = torch.as_tensor(timestep, device=dev)
        if t.ndim == 0:
            t = t[None]
        t = t.to(torch.float32).expand(B).contiguous()
        ehs = encoder_hidden_states.to(device=dev, dtype=torch.bfloat16).contiguous()
        L = ehs.shape[1]
        # B rows of text, or B * F in the per-frame form (FreeNoise prompt travel), video-major
        if ehs.dim() != 3 or ehs.shape[0] not in (B, B * Fr):
            raise ValueError(f"encoder_hidden_states of shape {tuple(ehs.shape)}: expected {B} rows (one per video) "
                             f"or {B * Fr} (one per frame, video-major) of [tokens, dim]")
        if ehs.shape[0] != B and getattr(self, "dist", None) is not None:
            raise NotImplementedError("per-frame text together with frame sharding (dist=) is not supported: "
                                      "the text row layout is per video")
        control = self._control_residuals(down_block_additional_residuals, mid_block_additional_residual,
                                          B * Fr, H, W)
        if self.has_hooks():
            out = self.forward_modules(sample.to(dev, torch.float32), t, ehs, control=control)
        else:
            te = ops.timestep_embed(t, self.time_proj.num_channels)
            ctx = self.make_ctx(te, ehs.reshape(ehs.shape[0] * L, -1), B, Fr, L)
            x_rows = ops.pack_latents(sample.to(dev), dup=1, cpad=CIN_PAD)
            eps_rows = self.forward_rows(x_rows, H, W, ctx, control=control)
            out = ops.unpack_nhwc(eps_rows, B, self.config["out_channels"], Fr, H, W)
        out = out.to(sample.dtype) if sample.dtype.is_floating_point else out
        return UNetMotionOutput(out) if return_dict else (out,)
