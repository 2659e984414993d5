"""Executor of the pruned / dense SD-2.1 U-Net: the dataflow of UNet2DConditionModelGated.forward
(pdm/models/unet/unet_2d_conditional.py:1417-1728) with the leaves of SURVEY Appendix B, over the op layer of ../ops.py
(explicit forward + hand-written backward, no autograd).  What is here is the U-Net's own: the training switches read
from the environment, the ResBlock / transformer / whole-model forward, the concat views that let a skip and its consumer
share one buffer, the block markers of the bucketed all-reduce, and the grouped weight gradients of a transformer block.
"""
import math
import os

import torch

from ... import _pdmk as k
from ..ops import Act, Ops
from .params import ParamStore, kv_layout, temb_layout
from .spec import UNetConfig, padc


class UNetEngine(Ops):
    def __init__(self, cfg: UNetConfig, blocks, store: ParamStore, dtype):
        # Linear weight gradients: splits store partial slabs, one grouped launch adds them (PDMK_WGRAD_SLABS=0: atomics)
        # (the 3x3 conv weight gradients keep the atomics: their slabs are sk x 4-60 MB each, measured 43.3 vs 43.6 ms per main step)
        slabs = k.SlabQueue() if os.environ.get("PDMK_WGRAD_SLABS", "1") != "0" else None
        super().__init__(
            store, dtype, norm_groups=cfg.norm_num_groups,
            fuse_geglu=os.environ.get("PDMK_FUSE_GEGLU", "1") != "0",     # A/B switch: 0 = projection + GEGLU as two passes
            # LayerNorm in the prologue of the Linear that reads it (linear(ln=...)): 0 = never, 1 = where it measured as a gain
            # (K <= 320, the 128-row register image: +2 ... +13 us per pair at M = 32 768; the 64-row image of K <= 640 loses
            # 0 ... 20 us to the ring kernels it displaces - tools/ln_fuse_bench.py), 2 = wherever the library takes the pair
            fuse_ln=int(os.environ.get("PDMK_FUSE_LN", "1")),
            fuse_geglu_bwd=os.environ.get("PDMK_FUSE_GEGLU_BWD", "1") != "0",   # same for the backward (ff.net.2's input gradient)
            defer_fanin=os.environ.get("PDMK_DEFER_FANIN", "1") != "0",   # A/B switch: 0 = residual gradients added at once
            # GroupNorm / LayerNorm affine gradients: the second-stage reductions of a whole block run as one launch at the
            # block boundary (PDMK_DEFER_PARTIALS=0: one launch per layer, as before)
            partials=k.PartialQueue() if os.environ.get("PDMK_DEFER_PARTIALS", "1") != "0" else None,
            slabs=slabs,
            # upsampler convs as four 2x2 phase convs on the low-resolution image (PDMK_CONV_UP2=0: nearest x2 fused into the
            # 3x3 gather, 2.25 x the multiply-accumulates)
            up2=os.environ.get("PDMK_CONV_UP2", "1") != "0",
            # GroupNorm statistics from the producing GEMM's epilogue (PDMK_GN_EPI=0: a statistics pass per GroupNorm).  The
            # per-(image, column) accumulators of one forward pass live in ONE arena zeroed by one launch at its start
            gn_epi=os.environ.get("PDMK_GN_EPI", "1") != "0" and dtype == torch.bfloat16,
            # Linear weight gradients of a transformer block: collected during the block's backward and issued as grouped launches
            # at its start marker (k.wgrad_group; PDMK_WGRAD_GROUP=0: one launch per weight, as they are produced)
            # (conv1 / conv2 of a ResBlock grouped the same way measured -0.3 ... +0.2 % for the step in three A/Bs and was removed)
            group_wgrad=os.environ.get("PDMK_WGRAD_GROUP", "1") != "0" and dtype == torch.bfloat16 and slabs is not None)
        # (attn_fp8, the "fp8_e4m3" attention precision - Q / K / V rounded to e4m3fn values - is set by
        # UNet2DConditionModelPruned.set_attention_precision)
        self.cfg, self.blocks = cfg, blocks
        half = cfg.block_out_channels[0] // 2
        # frequency table of Timesteps(dim, flip_sin_to_cos=True, shift=0): built exactly like the reference (fp32 exp)
        self.freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half).to(self.dev)
        self.grad_ready_cb = None      # called with an arena offset: every gradient at or beyond it is final
        self.temb_lay, self.temb_cols = temb_layout(cfg, blocks)
        self.kv_lay, self.kv_cols = kv_layout(blocks)
        # skip k (push order) is concatenated behind an h of cat_ch[k] channels (None: its consumer ResBlock is dropped)
        ups = [r for b in blocks if b.kind == "up" for r in b.resnets]
        self.cat_ch = [None if r.dropped else padc(r.cin - r.skip) for r in reversed(ups)]
        # feed-forward blocks in execution order (down, mid, up): the layer index an ffn_observer is called with
        self.ffn_index = {a.name: i for i, a in enumerate(a for b in blocks for a in b.attns if not a.dropped)}

    # ------------------------------------------------------------------ concat views
    def _skip_view(self, k_, M, C, B=0):
        """(buffer, view) for the producer of skip number k_ (push order): the right C columns of its concat buffer.  The
        buffer gets ONE GroupNorm accumulator for all its columns (both producers add their column sums to it)."""
        ch = self.cat_ch[k_] if k_ < len(self.cat_ch) else None
        if ch is None:
            return None, None
        cat = self._empty(M, ch + C)
        view = cat[:, ch:]
        if self.gn_epi and self._cs_shape_ok(M, B, ch + C) and self.dtype == torch.bfloat16:
            acc = self._cs_alloc(B, ch + C)
            self._cs_cats[cat.data_ptr()] = acc
            self._cs_views[view.data_ptr()] = (acc, ch, cat)
            if ch:
                self._cs_views[cat.data_ptr()] = (acc, 0, cat)
        return cat, view

    @staticmethod
    def _cs_shape_ok(M, B, ld):
        return B > 0 and M % B == 0 and (M // B) % 64 == 0 and ld % 8 == 0

    @staticmethod
    def _left_view(skips, M, C):
        """View for the producer of the h that the NEXT concat puts in front of the skip on top of the stack, or None."""
        if not skips or skips[-1][1] is None:
            return None
        s, cat = skips[-1]
        if cat.shape[0] != M or cat.shape[1] != C + s.t.shape[1]:
            return None
        return cat[:, :C]

    # ------------------------------------------------------------------ blocks
    def _mark(self, first_key):
        """Tape marker placed at the START of a block: it runs after the whole block's backward, i.e. when every
        gradient from this block's first arena entry to the end of the arena is final (bucketed all-reduce trigger)."""
        if self.train:
            off = self.P.by_key[first_key].off

            def mark():
                if self.grad_ready_cb:     # a consumer that acts on [off, total) calls flush_pending() first
                    self.grad_ready_cb(off)
            self.tape.append(mark)

    def resblock(self, x, r, st, B, H, W, out=None, cs=True):
        """cs: a GroupNorm reads this block's output directly (not through a concat): conv2's epilogue forms its statistics."""
        G = self.cfg.norm_num_groups
        p = r.name
        self._mark(p + ".norm1.weight")
        n1 = self.groupnorm(x, p + ".norm1", B, H * W, G, r.cin // G, 1e-5, True)
        h1, _, _ = self.conv3(n1, p + ".conv1", B, H, W, 0, p + ".conv1.bias", rowvec=st, rv_cols=self.temb_lay[p][:2], cs=True)
        n2 = self.groupnorm(h1, p + ".norm2", B, H * W, r.groups2(G), r.cout // G, 1e-5, True)
        res = x if r.cin == r.cout else self.linear(x, p + ".conv_shortcut", bias=p + ".conv_shortcut.bias")
        y, _, _ = self.conv3(n2, p + ".conv2", B, H, W, 0, p + ".conv2.bias", residual=res, out=out, cs=cs)
        return y

    def transformer(self, x, a, ehs, B, H, W, T, out=None, cs=True):
        G = self.cfg.norm_num_groups
        p, c, N = a.name, a.c, H * W
        t = p + ".transformer_blocks.0"
        d1, d2 = a.h1() * 64, a.h2() * 64
        self._mark(p + ".norm.weight")
        if self.train and self.group_wgrad:
            self.tape.append(self._wg_flush)       # runs at the end of the block's backward, before the mark above
        n = self.groupnorm(x, p + ".norm", B, N, G, c // G, 1e-6, False)
        h = self.linear(n, p + ".proj_in", bias=p + ".proj_in.bias")
        qkv = self.linear(h, t + ".attn1.to_qkv", ln=t + ".norm1")
        if self.attn_fp8:            # in place: the backward pass recomputes the scores from the same rounded operands
            k.quantize_e4m3_(qkv.t)
        o = self.attention(qkv.t[:, :d1], qkv.t[:, d1:2 * d1], qkv.t[:, 2 * d1:3 * d1], B, a.h1(), N, N, qkv, qkv,
                           (0, d1), ((d1, 2 * d1), (2 * d1, 3 * d1)))
        h = self.linear(o, t + ".attn1.to_out.0", bias=t + ".attn1.to_out.0.bias", residual=h)
        q = self.linear(h, t + ".attn2.to_q", ln=t + ".norm2")
        if self.attn_fp8:
            k.quantize_e4m3_(q.t)
        kv, ko = ehs, self.kv_lay[p][0]      # `ehs` = the batched K/V projection of all transformers; this one's columns
        o = self.attention(q.t[:, :d2], kv.t[:, ko:ko + d2], kv.t[:, ko + d2:ko + 2 * d2], B, a.h2(), N, T, q, kv, (0, d2),
                           ((ko, ko + d2), (ko + d2, ko + 2 * d2)))
        h = self.linear(o, t + ".attn2.to_out.0", bias=t + ".attn2.to_out.0.bias", residual=h)
        gl = self.linear(h, t + ".ff.net.0.proj", bias=t + ".ff.net.0.proj.bias", geglu=True, ln=t + ".norm3")
        if self.ffn_observer is not None:
            self.ffn_observer(self.ffn_index[p], gl.t)
        h = self.linear(gl, t + ".ff.net.2", bias=t + ".ff.net.2.bias", residual=h)
        y = self.linear(h, p + ".proj_out", bias=p + ".proj_out.bias", residual=x, out=out, cs=(B, N) if cs else None)
        if self.train and self.group_wgrad:
            self.tape.append(self._wg_open)        # runs first in the block's backward
        return y

    # ------------------------------------------------------------------ whole model
    def forward(self, x, timesteps, ehs, B, H, W, train):
        """x: [B*H*W, padc(in_channels)] NHWC rows in self.dtype; timesteps int64 [B], or float32 [B] for fractional ones
        (k.timestep_embed dispatches on the dtype); ehs: [B*T, ctx] in self.dtype.
        Returns (pred Act [B*H*W, padc(out_channels)], acts {d0..,m,u0..: Act})."""
        cfg = self.cfg
        self.train = train
        self.tape = []
        self._cs_begin()
        T = ehs.shape[0] // B
        c0 = cfg.block_out_channels[0]
        te = self._empty(B, c0)
        k.timestep_embed(timesteps, self.freqs, te, B, c0)
        e1 = self.linear(Act(te, rg=False), "time_embedding.linear_1", bias="time_embedding.linear_1.bias")
        temb = self.linear(self.silu(e1), "time_embedding.linear_2", bias="time_embedding.linear_2.bias")
        st = self.silu(temb)                      # shared by every ResBlock (blocks.py:336)
        if self.temb_cols:                        # all time_emb_proj in one skinny GEMM; ResBlocks take column slices
            st = self.linear(st, "time_emb_proj_all", bias="time_emb_proj_all.bias", out_f32=True)
        ehs_act = Act(ehs, rg=False)
        if self.kv_cols:                          # all cross-attention K/V projections in one GEMM; layers take column slices
            ehs_act = self.linear(ehs_act, "attn2_kv_all")
            ehs_act.rg = train
            if self.attn_fp8:        # the K / V of every cross attention, once
                k.quantize_e4m3_(ehs_act.t)
        c0p = padc(c0)
        nskip = 0

        def push(act, cat):         # (skip tensor, its concat buffer or None)
            nonlocal nskip
            skips.append((act, cat))
            nskip += 1

        skips = []
        cat, view = self._skip_view(nskip, B * H * W, c0p, B)
        h, _, _ = self.conv3(Act(x, rg=False), "conv_in", B, H, W, 0, "conv_in.bias", out=view, cs=True)
        push(h, cat)
        acts = {}
        for b in self.blocks:
            cb = padc(b.c)
            if b.kind == "down":
                for j, r in enumerate(b.resnets):
                    att = b.attns[j] if (b.attns and not b.attns[j].dropped) else None
                    cat, view = self._skip_view(nskip, B * H * W, cb, B)
                    made = False
                    if not r.dropped:
                        h = self.resblock(h, r, st, B, H, W, out=None if att is not None else view)
                        made = att is None
                    if att is not None:
                        h = self.transformer(h, att, ehs_act, B, H, W, T, out=view)
                        made = True
                    # both layers dropped: the skip IS the previous tensor, which has no concat buffer for this consumer
                    push(h, cat if made else None)
                if b.sampler:
                    cat, view = self._skip_view(nskip, B * ((H + 1) // 2) * ((W + 1) // 2), cb, B)
                    h, H, W = self.conv3(h, f"{b.name}.downsamplers.0.conv", B, H, W, 1,
                                         f"{b.name}.downsamplers.0.conv.bias", out=view, cs=True)
                    push(h, cat)
                acts[f"d{b.idx}"] = h
            elif b.kind == "mid":
                h = self.resblock(h, b.resnets[0], st, B, H, W)
                h = self.transformer(h, b.attns[0], ehs_act, B, H, W, T)
                h = self.resblock(h, b.resnets[1], st, B, H, W, out=self._left_view(skips, B * H * W, cb))
                acts["m"] = h
            else:
                n = len(b.resnets)
                for j, r in enumerate(b.resnets):
                    s, scat = skips.pop()
                    att = b.attns[j] if (b.attns and not b.attns[j].dropped) else None
                    # the tensor this pair leaves behind is the left half of the next concat (unless an upsampler follows)
                    nxt = None if (j == n - 1 and b.sampler) else self._left_view(skips, B * H * W, cb)
                    # (ahead of an upsampler no GroupNorm reads the tensor: no statistics for it)
                    last = j == n - 1 and b.sampler
                    if not r.dropped:      # dropped: keep the non-skip channels == h itself (blocks.py:502-515)
                        h = self.resblock(self.concat(h, s, scat), r, st, B, H, W, out=None if att is not None else nxt,
                                          cs=att is not None or not last)
                    if att is not None:
                        h = self.transformer(h, att, ehs_act, B, H, W, T, out=nxt, cs=not last)
                if b.sampler:
                    h, H, W = self.conv3(h, f"{b.name}.upsamplers.0.conv", B, H, W, 2,
                                         f"{b.name}.upsamplers.0.conv.bias",
                                         out=self._left_view(skips, B * 4 * H * W, cb), cs=True)
                acts[f"u{b.idx}"] = h
        assert not skips
        n = self.groupnorm(h, "conv_norm_out", B, H * W, cfg.norm_num_groups, c0 // cfg.norm_num_groups, 1e-5, True)
        pred, _, _ = self.conv3(n, "conv_out", B, H, W, 0, "conv_out.bias")
        return pred, acts
