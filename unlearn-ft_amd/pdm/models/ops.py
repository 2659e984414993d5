"""The op layer every model here runs on: launch wrappers of libpdmk over one `ParamStore`, with hand-written backward.

Activations are token-major / NHWC 2-D matrices [rows, C] (`Act`), so conv outputs feed Linear GEMMs and back without any
layout change.  With `train` set every op appends its backward closure to a tape; `backward()` replays the tape in reverse.
Gradients w.r.t. parameters are ACCUMULATED into the fp32 grad arena (zeroed by the fused AdamW).  Gradient fan-in
(residuals, skip connections, a shared operand) is owned by the gradient slot of `Act`: a kernel asks `dst()` where to write
and whether to accumulate, a finished buffer arrives through `give()`; the sums happen in GEMM / norm epilogues (accumulate
flags, addend ports) or by aliasing a finished buffer - there are no standalone "add" passes on the hot path.
`Ops(store, dtype)` alone is the inference configuration the VAE and both CLIP towers use; the U-Net's dataflow and its
training switches are `unet.engine.UNetEngine(Ops)`.  Every attribute a method here reads is set by `Ops.__init__`.
"""
import os
from collections import namedtuple

import torch

from .. import _pdmk as k


class Act:
    """A 2-D activation [rows, cols] (row stride = t.stride(0)) and the slot of its gradient (same logical shape).  The slot is
      empty   no gradient yet;
      owned   a buffer this Act may accumulate into - one a kernel wrote for it, or a finished buffer handed over by give()
              (ownership moves with it: the ResBlock residual is summed in place, which saves a pass);
      lent    a finished buffer a deferred weight gradient (Ops._wg_items) still reads: it may be read and passed as a kernel's
              addend, it is NEVER written - whatever would write it gets a private copy first (one copy2d) - until release();
      and an owned slot may carry a pending addend: a second finished buffer (the residual branch's, blocks.py:379) that the
      next GroupNorm / LayerNorm backward of this tensor folds into its own store (dst(port=True)) - so the fan-in normally costs
      no pass at all - or that the next read of `.g` adds (one strided accumulate pass)."""
    __slots__ = ("t", "rg", "src", "cs", "_g", "_add", "_lent")

    def __init__(self, t, rg=True):
        self.t, self.rg, self._g, self._add, self._lent = t, rg, None, None, False
        self.cs = None       # (accumulator [B, 2, ld], first column, columns covered): per-(image, column) sums of this tensor from
                             # its producers' epilogues (pdmk_gemm_args.colstat) - the GroupNorm that reads it skips its statistics pass
        self.src = None      # a GEGLU output: (pre-activation tensor, the projection's Act) - its consumer's input gradient can be
                             # pushed through GEGLU's backward in the GEMM epilogue (PDMK_EPI_GEGLU_BWD)

    @property
    def empty(self):
        """No gradient has arrived yet (nothing was written, given or seeded)."""
        return self._g is None

    @property
    def g(self):
        """The gradient, complete as far as the tape has run (a pending addend is added first).  A lent buffer is returned as it
        is - for reading."""
        self._fold()
        return self._g

    @g.setter
    def g(self, v):
        assert self._add is None and not self._lent
        self._g = v

    def _fold(self):
        if self._add is not None:
            a, self._add = self._add, None
            k.copy2d(a, self._g, a.shape[0], a.shape[1], a.stride(0), self._g.stride(0), accumulate=True)

    def _own(self):
        """lent -> owned: the private copy a writer needs (the lent buffer stays as the deferred weight gradient reads it)."""
        if self._lent:
            src, self._lent = self._g, False
            self._g = torch.empty(src.shape, device=src.device, dtype=self.t.dtype)
            k.copy2d(src, self._g, src.shape[0], src.shape[1], src.stride(0), self._g.stride(0))

    def dst(self, port=False):
        """Where a kernel writes d(self): (buffer, accumulate, addend).  port: the kernel can add a second tensor in the same
        store - it gets the pending addend, or the lent buffer (then it writes a fresh one); without a port addend is None."""
        add = None
        if port:
            add, self._add = self._add, None
            if self._lent:
                add, self._g, self._lent = self._g, None, False
        else:
            self._own()
        if self._g is None:
            self._g = torch.empty(self.t.shape, device=self.t.device, dtype=self.t.dtype)
            return self._g, False, add
        self._fold()
        return self._g, True, add

    def give(self, dy, lend=False, defer=False):
        """self.g += dy where dy is a finished gradient buffer: taken over when the slot is empty (lend: as a LENT buffer - dy
        is also the operand of a deferred weight gradient), else added - as the pending addend (defer) or by one accumulate pass."""
        if not self.rg:
            return
        if self._g is None:
            self._g, self._lent = dy, lend
            return
        self._own()             # a second finished gradient at a lent one: the sum gets a buffer of its own
        if defer and dy.dtype == self._g.dtype:
            self._fold()        # (an earlier pending addend goes in first)
            self._add = dy
        else:
            k.copy2d(dy, self._g, dy.shape[0], dy.shape[1], dy.stride(0), self._g.stride(0), accumulate=True)

    def release(self):
        """The launch that read the lent buffer has been issued: from here on it is owned like any handed-over buffer."""
        self._lent = False


def _ld(t):
    return t.stride(0)


# what the backward of one Linear call needs: weight and bias keys, shape, x = the input Act as the GEMM read it, out = the Act of
# the [M, N] output, the residual Act or None, the logical multiply-accumulates
_Lin = namedtuple("_Lin", "key bias M N K x out residual macs")


class Ops:
    def __init__(self, store, dtype, *, norm_groups=32, fuse_geglu=True, fuse_ln=0, fuse_geglu_bwd=False, defer_fanin=False,
                 partials=None, slabs=None, up2=False, gn_epi=False, group_wgrad=False, attn_fp8=False, ffn_observer=None):
        """The defaults are inference behaviour; what each switch selects is told where UNetEngine reads it from the
        environment (unet/engine.py).  ffn_observer: None, or a callable (layer index, tensor [M, F]) that the model calls with
        the input of every feed-forward output projection (ConceptPrune: pdm/utils/concept_prune.py)."""
        self.P, self.dtype = store, dtype
        self.dev = store.master.device
        self.ws = k.groupnorm_ws(self.dev, 64, norm_groups)      # GN scratch, regrown by groupnorm() if B asks for more
        self.tape = []
        self.train = False
        self.macs = 0
        self.count_macs = False
        self.fuse_geglu, self.fuse_ln, self.fuse_geglu_bwd, self.defer_fanin = fuse_geglu, fuse_ln, fuse_geglu_bwd, defer_fanin
        self.partials, self.slabs = partials, slabs              # k.PartialQueue / k.SlabQueue, or None: nothing deferred
        self.up2, self.gn_epi, self.group_wgrad, self.attn_fp8 = up2, gn_epi, group_wgrad, attn_fp8
        self.ffn_observer = ffn_observer
        self._wg_items = None          # a list while Linear weight gradients are being collected for one grouped launch
        self._wg_lent = []             # the Acts that hold a dy of those items as a lent buffer
        self.gn_count, self.gn_miss = [0, 0], None
        self._cs_arena, self._cs_off, self._cs_need, self._cs_max, self._cs_old = None, 0, 0, 0, []
        self._cs_views, self._cs_cats = {}, {}

    # ------------------------------------------------------------------ helpers
    def _empty(self, rows, cols, dtype=None):
        return torch.empty((rows, cols), device=self.dev, dtype=dtype or self.dtype)

    def _give(self, act, dy, lend=False):
        """act.g += the finished buffer dy (Act.give); lend: dy is an operand of a weight gradient waiting in _wg_items."""
        act.give(dy, lend, self.defer_fanin)
        if lend:
            self._wg_lent.append(act)

    def _wg_open(self):
        """From here on the Linear weight gradients are collected (a transformer block's backward starts)."""
        self._wg_items = []

    def _wg_flush(self, reopen=False):
        """One grouped launch for what was collected; the buffers it reads are no longer lent."""
        items, self._wg_items = self._wg_items, [] if reopen else None
        if items:
            k.wgrad_group(items, self.slabs)
        for act in self._wg_lent:
            act.release()
        self._wg_lent = []

    def flush_pending(self):
        """Deferred norm-affine gradient reductions (PartialQueue): after this every gradient the tape has produced so far is
        final in the arena.  Called by whoever consumes gradients mid-backward (bucketed all-reduce, streamed AdamW, graph
        cut) and at the end of backward()."""
        if self._wg_items:          # (a consumer in the middle of a transformer block: what was collected so far goes out now)
            self._wg_flush(reopen=True)
        if self.partials is not None:
            self.partials.flush()
        if self.slabs is not None:
            self.slabs.flush()

    # ------------------------------------------------------------------ ops
    def linear(self, x, key, bias=None, residual=None, out_f32=False, out=None, geglu=False, cs=None, ln=None):
        """ln: key prefix of a LayerNorm whose output this Linear reads (BasicTransformerBlock norm1/2/3, blocks.py:705-867): x is
        the UN-normalised tensor; where the library takes the pair as one launch (pdmk_gemm_args.ln_gamma: the row-block kernel
        normalises the row block in its registers) the LayerNorm has no pass of its own - the normalised rows and (mean, rstd) are
        written only when a backward pass will read them - else the LayerNorm runs first, as a launch of its own.
        out: optional [M, N] view (any row stride) to write into instead of a fresh tensor (concat buffers).
        geglu: the projection is GEGLU's (blocks.py:44-59; weight rows packed (hidden, gate)-interleaved, params.py): returns
        hidden * gelu(gate) [M, N/2], computed in the GEMM's epilogue where the library has the fused kernel (bf16 ring
        kernels; the pre-activation is then only written when a backward pass will need it), else as a second pass.
        The form is decided here, once: skinny, LayerNorm prologue, fused GEGLU (_lin_geglu) or planned (_lin_planned) forward,
        and _lin_bwd_skinny or _lin_bwd_tiled on the tape."""
        P = self.P
        e = P.by_key[key + ".weight"]
        N, K = e.shape
        M = x.t.shape[0]
        assert x.t.shape[1] == K, f"{key}: input has {x.t.shape[1]} cols, weight expects {K}"
        assert not geglu or (residual is None and out is None and not out_f32)
        y = out if out is not None else self._empty(M, N, torch.float32 if out_f32 else None)
        assert tuple(y.shape) == (M, N)
        w, b = P.wv(key + ".weight"), (P.p(bias) if bias else None)
        macs = M * e.logical[0] * e.logical[1]          # logical (un-pruned-padding) multiply-accumulates
        if self.count_macs:
            self.macs += macs
        # time-embedding MLP / batched time_emb_proj: M = batch rows -> weight-streaming kernels (skinny operand in LDS)
        skinny = M <= 16 and residual is None and (8 if M <= 8 else 16) * K * 4 + 512 <= 65536
        a, ln_args = x.t, None             # forward A operand; the LayerNorm prologue of the GEMM
        if ln is not None:
            if (self.fuse_ln and self.dtype == torch.bfloat16 and not skinny and residual is None and out is None and
                    not out_f32 and cs is None and (self.fuse_ln >= 2 or K <= 320) and
                    k.gemm_ln_supported(a, w, M, N, K, _ld(a), K, geglu=geglu, bias=bool(bias))):
                x, ln_args = self._ln_prologue(x, ln)
            else:
                x = self.layernorm(x, ln)
                a = x.t
        c = _Lin(key, bias, M, N, K, x, None, residual, macs)
        gl, acc = (self._empty(M, N // 2) if geglu else None), None
        # fused GEGLU where configuration and plan allow it; the library may still refuse the shape: two passes then
        if (geglu and self.fuse_geglu and not skinny and self.dtype == torch.bfloat16 and
                (ln_args is not None or k.splitk_plan(a, w, M, N, K, _ld(a), K) == 1) and self._lin_geglu(c, a, w, b, gl, y, ln_args)):
            if not self.train:
                y = None                        # inference (teacher): the [M, N] pre-activation never reached memory
        else:
            if ln_args is not None:             # LayerNorm prologue: one kernel family, no plan to make
                k.gemm(a, w, y, M, N, K, _ld(a), K, _ld(y), bias=b, macs=macs, ln=ln_args)
            elif skinny:
                k.skinny_gemm(a, w, y, M, N, K, _ld(a), K, _ld(y), bias=b)
            else:
                acc = self._lin_planned(c, a, w, b, y, out_f32, cs, out is not None)
            if geglu:
                k.geglu_fwd(y, gl, M, N // 2, _ld(y), N // 2, layout=1)
        out = Act(y)
        c = c._replace(out=out)
        if acc is not None:
            out.cs = (acc[0], acc[1], N)
        if self.train:
            self.tape.append((lambda: self._lin_bwd_skinny(c)) if skinny else (lambda: self._lin_bwd_tiled(c)))
        if not geglu:
            return out
        act = Act(gl)
        if self.train:
            act.src = (y, out)

            def gbwd():               # runs BEFORE the projection's own backward: d(pre-activation) from d(gl)
                if out.empty:         # else: already produced by the consumer's fused epilogue (PDMK_EPI_GEGLU_BWD)
                    out.g = self._empty(M, N)
                    k.geglu_bwd(y, act.g, out.g, M, N // 2, _ld(y), _ld(act.g), N, layout=1)
            self.tape.append(gbwd)
        return act

    def _ln_prologue(self, src, ln):
        """The LayerNorm `ln` of src leaves with the GEMM that reads it: returns (the Act the Linear's backward sees as its input,
        the ln tuple of k.gemm).  The normalised rows and the statistics are written only for a backward pass."""
        P = self.P
        M, K = src.t.shape
        st_ = torch.empty((M, 2), device=self.dev, dtype=torch.float32) if self.train else None
        x = Act(self._empty(M, K) if self.train else None)
        if self.train:
            def lnbwd():                             # runs AFTER the Linear's backward (appended before it)
                dx, acc, add = src.dst(port=True)
                k.layernorm_bwd(src.t, x.g, dx, P.p(ln + ".weight"), st_, P.g(ln + ".weight"), P.g(ln + ".bias"), M, K, _ld(src.t),
                                _ld(x.g), _ld(dx), acc, queue=self.partials, add=add)
            self.tape.append(lnbwd)
        return x, (P.p(ln + ".weight"), P.p(ln + ".bias"), st_, x.t, 1e-5)

    def _lin_geglu(self, c, a, w, b, gl, y, ln_args):
        """Fused GEGLU epilogue (with or without the LayerNorm prologue): gl and, when training, the pre-activation y are written
        by one launch.  False: the library has no fused kernel for the shape, nothing was launched."""
        fused = k.gemm_geglu(a, w, gl, y if self.train else None, c.M, c.N, c.K, _ld(a), c.K, bias=b, macs=c.macs, ln=ln_args)
        assert fused or ln_args is None, "pdmk_gemm_ln_supported said yes"
        return fused

    def _lin_planned(self, c, a, w, b, y, out_f32, cs, view):
        """Planned GEMM (+ bias, residual).  cs = (B, rows per image): a GroupNorm reads this output next - its statistics come
        out of this epilogue; returns their (accumulator, first column) when they were fed, else None."""
        R, ldr = (c.residual.t, _ld(c.residual.t)) if c.residual else (None, 0)
        if out_f32:
            k.gemm(a, w, y, c.M, c.N, c.K, _ld(a), c.K, _ld(y), bias=b, R=R, ldr=ldr, macs=c.macs, out_f32=True)
            return None
        acc = self._cs_for(y, cs[0], cs[1], c.M, c.N, view=view) if cs is not None else None
        got = k.gemm_auto(a, w, y, c.M, c.N, c.K, _ld(a), c.K, _ld(y), bias=b, R=R, ldr=ldr, macs=c.macs,
                          **({"colstat": acc, "rows_per_b": cs[1]} if acc is not None else {}))
        return acc if got else None

    def _lin_bwd_skinny(self, c):
        P, M, N, K, x = self.P, c.M, c.N, c.K, c.x
        dy = c.out.g
        k.skinny_wgrad(dy, x.t, P.g(c.key + ".weight"), P.g(c.bias) if c.bias else None, M, N, K, _ld(dy), _ld(x.t), K)
        if not x.rg:
            return
        wt = P.wtv(c.key + ".weight")
        if (8 if M <= 8 else 16) * N * 4 + 512 <= 65536:      # dy fits LDS too
            dx, acc, _ = x.dst()
            k.skinny_gemm(dy, wt, dx, M, K, N, _ld(dy), N, _ld(dx), accumulate=acc)
        else:                     # wide projection (all time_emb_proj at once): dy does not fit LDS -> tiled GEMM
            dy = self._as_dtype(dy, M, N)
            dx, acc, _ = x.dst()
            k.gemm_auto(dy, wt, dx, M, K, N, N, N, _ld(dx), accumulate=acc, macs=c.macs)

    def _as_dtype(self, dy, M, N):
        """dy in the compute dtype (fp32 outputs - the time-embedding projections: a tiny cast for the GEMMs)."""
        if dy.dtype == self.dtype:
            return dy
        dyc = self._empty(M, N)
        k.cast_permute(dy, dyc, M * N, 1, 1, 0)
        return dyc

    def _lin_bwd_tiled(self, c):
        P, M, N, K, x = self.P, c.M, c.N, c.K, c.x
        dy = self._as_dtype(c.out.g, M, N)
        wt = P.wtv(c.key + ".weight")
        item = k.WgradItem(dy=dy, x=x.t, dW=P.g(c.key + ".weight"), M=N, N=K, K=M, lda=_ld(dy), ldb=_ld(x.t),
                           colsum_out=P.g(c.bias) if c.bias else None, macs=c.macs)     # (the bias gradient is fused in)
        collect = self._wg_items is not None
        if collect:      # inside a transformer block: the weight gradient joins the block's grouped launch (dy and x.t stay
            self._wg_items.append(item)        # referenced - and unmodified: dy is LENT to the residual below - until _wg_flush)
        else:
            k.wgrad(*item[:8], colsum_out=item.colsum_out, macs=item.macs, queue=self.slabs)
        fused = False
        if (x.rg and x.src is not None and x.empty and self.fuse_geglu_bwd and self.dtype == torch.bfloat16 and
                k.splitk_plan(dy, wt, M, K, N, _ld(dy), N) == 1):
            pre, proj = x.src          # gradient of the GEGLU pre-activation straight from this GEMM's epilogue
            dpre = self._empty(M, 2 * K)
            fused = k.gemm_geglu_bwd(dy, wt, pre, dpre, M, K, N, _ld(dy), N, macs=c.macs)
            if fused:
                proj.g = dpre
        if x.rg and not fused:
            dx, acc, _ = x.dst()
            k.gemm_auto(dy, wt, dx, M, K, N, _ld(dy), N, _ld(dx), accumulate=acc, macs=c.macs)
        if c.residual is not None:
            self._give(c.residual, c.out.g, lend=collect)

    def conv3(self, x, key, B, Hi, Wi, mode, bias, rowvec=None, residual=None, rv_cols=None, out=None, cs=False):
        """3x3 conv, pad 1.  mode 0: stride 1; 1: stride 2; 2: nearest-x2 upsample fused into the gather; 4: stride 2
        padded on the bottom/right only (VAE encoder downsample; forward only).
        rowvec (+ rv_cols = (first column, width)): per-image row added to every pixel = this ResBlock's column slice of
        the batched time-embedding projection [B, sum of widths] (fp32)."""
        P = self.P
        e = P.by_key[key + ".weight"]
        Cop, _, Cip = e.shape
        assert x.t.shape[1] == Cip, f"{key}: input has {x.t.shape[1]} channels, weight expects {Cip}"
        Ho, Wo = ((Hi + 1) // 2, (Wi + 1) // 2) if mode in (1, 4) else ((2 * Hi, 2 * Wi) if mode == 2 else (Hi, Wi))
        M = B * Ho * Wo
        y = out if out is not None else self._empty(M, Cop)
        assert tuple(y.shape) == (M, Cop)
        if (mode == 2 and self.up2 and rowvec is None and residual is None and
                k.conv_up2_supported(B, Hi, Wi, Cip, Cop, self.dtype)):
            return self._conv_up2(x, key, B, Hi, Wi, bias, y, e, cs and ("view" if out is not None else "own")), Ho, Wo
        acc = self._cs_for(y, B, Ho * Wo, M, Cop, view=out is not None) if cs else None   # a GroupNorm reads this output next
        lmacs = M * e.logical[0] * e.logical[1] * 9
        acc_ok = k.gemm_auto(x.t, P.wv(key + ".weight"), y, M, Cop, 9 * Cip, 0, 9 * Cip, _ld(y), a_mode=k.A_CONV,
               conv=(B, Hi, Wi, Cip, Ho, Wo, mode, _ld(x.t)), bias=P.p(bias),
               rowvec=rowvec.t[:, rv_cols[0]:] if rowvec is not None else None, rows_per_b=Ho * Wo,
               ldrv=_ld(rowvec.t) if rowvec is not None else 0,
               R=residual.t if residual else None, ldr=_ld(residual.t) if residual else 0, macs=lmacs, colstat=acc)
        if self.count_macs:
            self.macs += lmacs
        out = Act(y)
        if acc is not None and acc_ok:
            out.cs = (acc[0], acc[1], Cop)
        if self.train:
            def bwd():
                dy = out.g
                ldy = _ld(dy)
                xt = x.t
                k.wgrad(dy, xt, P.g(key + ".weight"), Cop, 9 * Cip, M, ldy, 0, b_mode=k.B_COLK_CONV,
                        conv=(B, Hi, Wi, Cip, Ho, Wo, mode, _ld(xt)), macs=lmacs,
                        colsum_out=P.g(bias))       # bias gradient fused into the weight gradient; splits add with atomics
                if x.rg:
                    if mode == 2:
                        self._dgrad_up2_pooled(x, dy, key, B, Hi, Wi, Cip, Cop, lmacs)
                    else:
                        dx, acc, _ = x.dst()
                        k.gemm_auto(dy, P.wtv(key + ".weight"), dx, B * Hi * Wi, Cip, 9 * Cop, 0, 9 * Cop, _ld(dx),
                                    a_mode=k.A_CONV, conv=(B, Ho, Wo, Cop, Hi, Wi, 3 if mode == 1 else 0, ldy),
                               accumulate=acc, macs=lmacs)
                if rowvec is not None:
                    # d(rowvec)[b] = column sums of dy over the pixels of image b, written into this block's column slice
                    # of the batched projection's gradient (the conv bias gradient - their sum over b - comes out of the weight
                    # gradient kernel)
                    if rowvec.empty:
                        rowvec.g = k.zeros(tuple(rowvec.t.shape), self.dev, torch.float32)
                    dtp = rowvec.g[:, rv_cols[0]:]
                    hw = Ho * Wo
                    # (accumulate: the slice was zeroed with the whole gradient above and is written once per backward pass - no
                    # zero-fill launch per ResBlock)
                    k.colsum(dy, dtp, hw, Cop, ldy, accumulate=True, nbatch=B, ldo=_ld(rowvec.g))
                if residual is not None:
                    self._give(residual, dy)
            self.tape.append(bwd)
        return out, Ho, Wo

    def _dgrad_up2_pooled(self, x, dy, key, B, Hi, Wi, Ci, Co, macs):
        """Input gradient of the nearest-x2 + 3x3 conv in its 3x3 form: at the high resolution, then summed 2x2 onto x's grid."""
        tmp = self._empty(4 * B * Hi * Wi, Ci)
        k.gemm_auto(dy, self.P.wtv(key + ".weight"), tmp, 4 * B * Hi * Wi, Ci, 9 * Co, 0, 9 * Co, Ci, a_mode=k.A_CONV,
                    conv=(B, 2 * Hi, 2 * Wi, Co, 2 * Hi, 2 * Wi, 0, _ld(dy)), macs=macs)
        pooled = self._empty(B * Hi * Wi, Ci)
        k.pool2x2_sum(tmp, pooled, B, Hi, Wi, Ci)
        self._give(x, pooled)

    def _conv_up2(self, x, key, B, Hi, Wi, bias, y, e, cs=False):
        """Upsample2D (nearest x2 + 3x3 conv; unet_2d_conditional.py up blocks) as four 2x2 phase convs
        on the low-resolution image (pdmk.h conv_mode 5..12): 16 instead of 36 multiply-accumulates per low-resolution pixel,
        forward, input gradient and weight gradient alike.  The four phases of the forward and of the weight gradient are
        independent problems of one shape: one grouped launch each (pdmk_gemm_group)."""
        P = self.P
        Cop, _, Cip = e.shape
        Ml = B * Hi * Wi
        wp, wpt = P.up2_weights(key)
        lmacs = 4 * Ml * e.logical[0] * e.logical[1] * 4           # executed multiply-accumulates
        mac9 = lmacs * 9 // 4                                      # (the 3x3 form, which is also how the reference executes and counts it)
        geo = lambda m, ci, ld: (B, Hi, Wi, ci, Hi, Wi, m, ld)
        # cs: False = no GroupNorm reads this output; "own" = y is a fresh tensor; "view" = y is a concat view (the four phases add
        # their column sums to that buffer's GroupNorm accumulator; rows are counted on the low-resolution grid a phase enumerates)
        acc = self._cs_for(y, B, Hi * Wi, Ml, Cop, view=cs == "view") if cs else None
        with k.Recorder() as r:
            for p_ in range(4):
                k.gemm(x.t, wp[p_], y, Ml, Cop, 4 * Cip, 0, 4 * Cip, _ld(y), a_mode=k.A_CONV, conv=geo(5 + p_, Cip, _ld(x.t)),
                       bias=P.p(bias), macs=lmacs // 4, colstat=acc, rows_per_b=Hi * Wi if acc is not None else 0)
        k.gemm_group(r.recs)
        if self.count_macs:
            self.macs += mac9
        out = Act(y)
        if acc is not None:
            out.cs = (acc[0], acc[1], Cop)
        if self.train:
            def bwd():
                dy = out.g
                ldy = _ld(dy)
                xt = x.t
                # small low-resolution grids (8x8 -> 16x16 at B = 8: 512 pixels) leave the phase forms of the two gradients with
                # too few workgroups: there the 3x3 forms at the high resolution stay (same arithmetic, measured faster -
                # tools/up2_bench.py)
                # (one MI355X, B = 8, us: weight gradient 32->64 329 -> 262, 16->32 329 -> 279, 8->16 98 -> 145; input gradient
                # 32->64 221 -> 134, 16->32 207 -> 204, 8->16 76 -> 203; forward 301 -> 139, 248 -> 123, 80 -> 55)
                phase_w, phase_d = Ml >= 2048, Ml >= 8192
                if phase_w:
                    # weight gradient: four phase problems into a zeroed [4][Co][4 Ci] buffer, then folded into the 3x3 gradient
                    dwp = k.zeros((4, Cop, 4 * Cip), self.dev, torch.float32)
                    sk = k.wgrad_plan(dy, xt, Cop, 4 * Cip, Ml, ldy, 0, k.B_COLK_CONV, geo(5, Cip, _ld(xt)))
                    with k.Recorder() as rw:
                        for p_ in range(4):
                            k.gemm(dy, xt, dwp[p_], Cop, 4 * Cip, Ml, ldy, 0, 4 * Cip, a_mode=k.A_COLK, b_mode=k.B_COLK_CONV,
                                   conv=geo(5 + p_, Cip, _ld(xt)), out_f32=True, splitk=sk, accumulate=(sk == 1),
                                   dtype=k.dt(xt), colsum_out=P.g(bias), macs=lmacs // 4)
                    k.gemm_group(rw.recs)
                    k.up2_combine_wgrad(dwp, P.g(key + ".weight"), Cop, Cip)
                else:
                    k.wgrad(dy, xt, P.g(key + ".weight"), Cop, 9 * Cip, 4 * Ml, ldy, 0, b_mode=k.B_COLK_CONV,
                            conv=(B, Hi, Wi, Cip, 2 * Hi, 2 * Wi, 2, _ld(xt)), macs=mac9, colsum_out=P.g(bias))
                if x.rg and phase_d:
                    # input gradient: all four phases as ONE problem (conv_mode 13: K = (phase, tap, channel))
                    dx, acc, _ = x.dst()
                    k.gemm(dy, wpt, dx, Ml, Cip, 16 * Cop, 0, 16 * Cop, _ld(dx), a_mode=k.A_CONV, conv=geo(13, Cop, ldy),
                           accumulate=acc, macs=lmacs)
                elif x.rg:
                    self._dgrad_up2_pooled(x, dy, key, B, Hi, Wi, Cip, Cop, mac9)
            self.tape.append(bwd)
        return out

    def _cs_begin(self):
        """Start of a forward pass: one zero fill for every GroupNorm accumulator of the pass."""
        self.gn_count = [0, 0]
        self.gn_miss = [] if os.environ.get("PDMK_GN_EPI_DEBUG") else None    # (layer, rows, columns) of GroupNorms without them
        if not self.gn_epi:
            return
        # sized for the LARGEST pass seen so far (the teacher alternates B and 2B passes): after one eager pass of every shape -
        # the warm-up that precedes any capture - the arena never grows again, so no capture allocates or zero-fills piecemeal
        self._cs_max = max(self._cs_max, self._cs_need)
        if self._cs_max and (self._cs_arena is None or self._cs_arena.numel() < self._cs_max):
            # grow: the old arena is RETAINED - a captured graph of an earlier (smaller) pass still zeroes and adds into it
            self._cs_old.append(self._cs_arena)
            self._cs_arena = torch.empty(max(self._cs_max, 1 << 16), device=self.dev, dtype=torch.int64)
        self._cs_off, self._cs_need = 0, 0
        self._cs_views, self._cs_cats = {}, {}
        if self._cs_arena is not None:
            k.zero_(self._cs_arena)

    def _cs_alloc(self, B, cols):
        """Zeroed accumulator [B, 4, cols] (int64 limbs, pdmk.h colstat; a slice of the pass's arena; the first pass of a new shape sizes the arena and
        zeroes its accumulators one by one)."""
        n = B * 4 * cols
        self._cs_need += n
        if self._cs_arena is not None and self._cs_off + n <= self._cs_arena.numel():
            t = self._cs_arena[self._cs_off:self._cs_off + n].view(B, 4, cols)
            self._cs_off += n
            return t
        return k.zeros((B, 4, cols), self.dev, torch.int64)

    def _cs_for(self, y, B, rows_per_b, M, N, view=False):
        """(accumulator [B, 4, ld], first column) for a GEMM that writes `y` [M, N] and whose output a GroupNorm reads next -
        or None when the statistics epilogue cannot take the shape (the GroupNorm then runs its own statistics pass).
        view: y is a concat-buffer view handed out by _skip_view / _left_view - the sums go to that buffer's accumulator, at the
        view's columns, so that the GroupNorm over the whole concat finds both halves in one place."""
        if not (self.gn_epi and rows_per_b > 0 and rows_per_b % 64 == 0 and M % 64 == 0 and N % 8 == 0 and
                y.stride(0) % 8 == 0 and y.dtype == torch.bfloat16):
            return None
        if view:
            # keyed by the view's address, and checked against the concat buffer it was registered for (which the entry keeps
            # alive, so the address cannot be recycled inside the pass): same rows, same row stride, columns inside the buffer
            ent = self._cs_views.get(y.data_ptr())
            if (ent is not None and ent[0].shape[0] == B and ent[1] + N <= ent[0].shape[2] and ent[2].shape[0] == y.shape[0] and
                    ent[2].stride(0) == y.stride(0)):
                return ent[0], ent[1]
        return self._cs_alloc(B, N), 0

    def groupnorm(self, x, key, B, HW, G, gs, eps, silu):
        P = self.P
        C = x.t.shape[1]
        y = self._empty(B * HW, C)
        stats = torch.empty((B, G, 2), device=self.dev, dtype=torch.float32)
        gw, gb = P.p(key + ".weight"), P.p(key + ".bias")
        cs = x.cs
        self.gn_count[0] += 1
        if cs is None and self.gn_miss is not None:
            self.gn_miss.append((key, B * HW, C))
        if cs is not None and cs[2] >= G * gs and cs[0].shape[0] == B:
            self.gn_count[1] += 1
            k.groupnorm_apply_colstat(x.t, y, gw, gb, stats, cs[0], cs[1], B, HW, C, _ld(x.t), C, G, gs, eps, silu)
        else:
            self.ws = k.groupnorm_ws(self.dev, B, G, self.ws)
            k.groupnorm_fwd(x.t, y, gw, gb, stats, self.ws, B, HW, C, _ld(x.t), C, G, gs, eps, silu)
        out = Act(y)
        if self.train:
            def bwd():
                dy = out.g
                dx, acc, add = x.dst(port=True)
                k.groupnorm_bwd(x.t, dy, dx, gw, gb, stats, P.g(key + ".weight"), P.g(key + ".bias"), self.ws, B,
                                HW, C, _ld(x.t), _ld(dy), _ld(dx), G, gs, silu, acc, add=add, queue=self.partials)
            self.tape.append(bwd)
        return out

    def layernorm(self, x, key):
        P = self.P
        M, C = x.t.shape
        y = self._empty(M, C)
        stats = torch.empty((M, 2), device=self.dev, dtype=torch.float32)
        gw = P.p(key + ".weight")
        k.layernorm_fwd(x.t, y, gw, P.p(key + ".bias"), stats, M, C, _ld(x.t), C, 1e-5)
        out = Act(y)
        if self.train:
            def bwd():
                dx, acc, add = x.dst(port=True)     # add: the residual branch's finished gradient
                k.layernorm_bwd(x.t, out.g, dx, gw, stats, P.g(key + ".weight"), P.g(key + ".bias"), M, C, _ld(x.t),
                                _ld(out.g), _ld(dx), acc, queue=self.partials, add=add)
            self.tape.append(bwd)
        return out

    def attention(self, q, kk, v, B, H, Nq, Nk, q_act, kv_act, q_cols, kv_cols):
        """q/kk/v: 2-D views [B*N, H*64] (column slices of the projection outputs); *_act own the gradients;
        q_cols / kv_cols = (lo, hi) column ranges of q in q_act and of (k, v) in kv_act."""
        d = H * 64
        o = self._empty(B * Nq, d)
        lse = torch.empty((B, H, Nq), device=self.dev, dtype=torch.float32)
        qs, ks, vs = (Nq * _ld(q), _ld(q)), (Nk * _ld(kk), _ld(kk)), (Nk * _ld(v), _ld(v))
        os_ = (Nq * d, d)
        scale = 64 ** -0.5
        k.attn_fwd(q, kk, v, o, lse, B, H, Nq, Nk, qs, ks, vs, os_, scale)
        if self.count_macs:
            self.macs += 2 * B * H * Nq * Nk * 64
        out = Act(o)
        if self.train:
            def bwd():
                delta = torch.empty((B, H, Nq), device=self.dev, dtype=torch.float32)
                if q_act.g is None:
                    q_act.g = self._empty(*q_act.t.shape)
                if kv_act.rg and kv_act.g is None:
                    kv_act.g = self._empty(*kv_act.t.shape)
                dq = q_act.g[:, q_cols[0]:q_cols[1]]
                if kv_act.rg:
                    dk = kv_act.g[:, kv_cols[0][0]:kv_cols[0][1]]
                    dv = kv_act.g[:, kv_cols[1][0]:kv_cols[1][1]]
                else:      # text conditioning does not need gradients, but the kernel writes dK/dV: scratch
                    scratch = self._empty(B * Nk, 2 * d)
                    dk, dv = scratch[:, :d], scratch[:, d:]
                k.attn_bwd(q, kk, v, o, out.g, lse, delta, dq, dk, dv, B, H, Nq, Nk, qs, ks, vs, os_,
                           (Nq * _ld(dq), _ld(dq)), (Nk * _ld(dk), _ld(dk)), (Nk * _ld(dv), _ld(dv)), scale)
            self.tape.append(bwd)
        return out

    def geglu(self, x):
        M, F2 = x.t.shape
        Fd = F2 // 2
        y = self._empty(M, Fd)
        k.geglu_fwd(x.t, y, M, Fd, _ld(x.t), Fd)
        out = Act(y)
        if self.train:
            def bwd():
                assert x.g is None
                x.g = self._empty(M, F2)
                k.geglu_bwd(x.t, out.g, x.g, M, Fd, _ld(x.t), _ld(out.g), F2)
            self.tape.append(bwd)
        return out

    def silu(self, x):
        y = torch.empty_like(x.t)
        k.silu_fwd(x.t, y)
        out = Act(y)
        if self.train:
            def bwd():
                assert x.g is None and out.g.is_contiguous()
                x.g = torch.empty_like(x.t)
                k.silu_bwd(x.t, out.g, x.g)
            self.tape.append(bwd)
        return out

    def concat(self, a, b, cat=None):
        """torch.cat([a, b], dim=1) of the up path.  `cat` = the [M, Ca + Cb] buffer whose right columns the
        skip b is a view of (its producer wrote them in place); a was normally written into the left columns by ITS producer
        (`out=`), so no copy happens at all; whatever is not in place yet is copied in."""
        M, Ca, Cb = a.t.shape[0], a.t.shape[1], b.t.shape[1]
        if cat is not None and tuple(cat.shape) != (M, Ca + Cb):
            cat = None
        inplace = cat is not None
        if cat is None:
            cat = self._empty(M, Ca + Cb)
            k.copy2d(b.t, cat[:, Ca:], M, Cb, _ld(b.t), Ca + Cb)
        if not (a.t.data_ptr() == cat.data_ptr() and _ld(a.t) == Ca + Cb):
            k.copy2d(a.t, cat, M, Ca, _ld(a.t), Ca + Cb)
            inplace = False
        out = Act(cat)
        acc = self._cs_cats.get(cat.data_ptr()) if inplace else None
        if (acc is not None and a.cs is not None and b.cs is not None and a.cs[0].data_ptr() == acc.data_ptr() and
                b.cs[0].data_ptr() == acc.data_ptr() and a.cs[1:] == (0, Ca) and b.cs[1:] == (Ca, Cb)):
            out.cs = (acc, 0, Ca + Cb)        # both producers summed into this buffer's accumulator: norm1 has its statistics
        if self.train:
            def bwd():
                self._give(a, out.g[:, :Ca])
                self._give(b, out.g[:, Ca:])
            self.tape.append(bwd)
        return out

    def backward(self):
        """Replays the tape; the caller has seeded .g of the loss inputs (pred and, optionally, block activations)."""
        tape, self.tape = self.tape, []
        for fn in reversed(tape):
            fn()
        self.flush_pending()
