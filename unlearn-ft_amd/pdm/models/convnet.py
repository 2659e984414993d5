"""What the convolutional evaluation networks on libpdmk share (Inception-v3 for FID, AlexNet for LPIPS, VGG-19 for the
style / content loss, ResNet-50 for the object-erasure accuracy): the unit record, the NHWC activation view, the host
helpers of their weight files (no GPU needed) and `ConvTrunk`, the base class of the models.  fp32, inference only.

A trunk keeps every weight in one fp32 arena - per unit the weight [Co, kh * kw * Ci] (k = (ky, kx, ci)) then the bias [Co],
each on a 512-byte line, further vectors behind them - and runs every conv as one pdmk_conv2d_fwd launch (implicit GEMM on
exact-fp32 MFMA, bias and ReLU in the epilogue; pdmk_conv2d_fwd_res adds a residual before the ReLU), eager on the current
stream.  How a unit maps to state-dict keys, and the forward pass, are each network's own (its spec.py and model module).
"""
import os
from dataclasses import dataclass

import torch

BN_FIELDS = ("weight", "bias", "running_mean", "running_var")


@dataclass(frozen=True)
class ConvUnit:
    name: str       # the unit's key in a trunk's `units` / `offsets`; its state-dict keys are the spec's business
    ci: int
    co: int
    kh: int = 1
    kw: int = 1
    stride: int = 1
    ph: int = 0
    pw: int = 0

    @property
    def k(self):
        return self.kh * self.kw * self.ci


class Map:
    """An NHWC activation: t is a 2-D view [B * H * W, C] of a buffer whose row stride may be wider than C."""

    def __init__(self, t, B, H, W):
        self.t, self.B, self.H, self.W, self.C, self.ld = t, B, H, W, t.shape[1], t.stride(0)


# ---- host helpers
def fold_batchnorm(w, gamma, beta, mean, var, eps):
    """Eval-mode BatchNorm folded into the conv in float64: (w * g / sqrt(var + eps), beta - mean * g / sqrt(var + eps)),
    both float64 (the caller rounds to fp32 once)."""
    w, gamma, beta, mean, var = (t.detach().to(torch.float64).cpu() for t in (w, gamma, beta, mean, var))
    s = gamma / torch.sqrt(var + eps)
    return w * s.reshape(-1, 1, 1, 1), beta - mean * s


def fold_unit(sd, conv, bn, eps):
    """fold_batchnorm of the conv `<conv>.weight` and the BatchNorm `<bn>.*` of a state dict."""
    return fold_batchnorm(sd[f"{conv}.weight"], *(sd[f"{bn}.{s}"] for s in BN_FIELDS), eps)


def conv_bn_shapes(units, keys, num_batches_tracked=True):
    """{key: shape} of conv (no bias) + BatchNorm units; keys(unit) -> (conv prefix, BatchNorm prefix)."""
    out = {}
    for u in units:
        conv, bn = keys(u)
        out[f"{conv}.weight"] = (u.co, u.ci, u.kh, u.kw)
        for s in BN_FIELDS:
            out[f"{bn}.{s}"] = (u.co,)
        if num_batches_tracked:
            out[f"{bn}.num_batches_tracked"] = ()
    return out


def checked(sd, want, what, ignored=None):
    """The tensors of `want` ({key: shape}) out of `sd`: a missing key raises KeyError and a mis-shaped one ValueError, both
    naming it.  ignored: None - every other key is ignored; else a predicate, and a key that is neither wanted nor ignored
    raises KeyError."""
    if ignored is not None:
        extra = [n for n in sd if n not in want and not ignored(n)]
        if extra:
            raise KeyError(f"unexpected keys in the {what} state dict: {sorted(extra)[:5]}")
    for n, shape in want.items():
        if n not in sd:
            raise KeyError(f"missing key {n} in the {what} state dict")
        if tuple(sd[n].shape) != tuple(shape):
            raise ValueError(f"{n}: shape {tuple(sd[n].shape)}, expected {tuple(shape)} ({what})")
    return {n: sd[n] for n in want}


def hub_checkpoint(name):
    """Where torch hub keeps a downloaded checkpoint of that file name."""
    return os.path.join(os.path.expanduser("~"), ".cache", "torch", "hub", "checkpoints", name)


def load_weights_file(path, name, flag, source):
    """The state dict of the file given, else of torch hub's cached `name`; never fetched."""
    path = path or hub_checkpoint(name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{source} weights not found at {path}: place {name} there or pass {flag} FILE "
                                f"(nothing is downloaded)")
    return torch.load(path, map_location="cpu", weights_only=True)


def arena_layout(units, extra=None):
    """({unit name: (weight offset, bias offset), extra name: offset}, size) in floats: every unit's weight then bias, then
    the vectors of `extra` ({name: length}), each on a 512-byte line."""
    def line(n):
        return (n + 127) // 128 * 128
    off, offsets = 0, {}
    for u in units:
        offsets[u.name] = (off, off + line(u.co * u.k))
        off = offsets[u.name][1] + line(u.co)
    for n, length in (extra or {}).items():
        offsets[n] = off
        off += line(length)
    return offsets, off


class ConvTrunk:
    """units: the ConvUnits of the arena (`units`, `offsets` by name); extra: further fp32 vectors {name: length}."""

    def __init__(self, device, units, extra=None):
        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} (MI355X engine) needs a GPU; there is no CPU fallback")
        self.device = torch.device(device or "cuda:0")
        self.units = {u.name: u for u in units}
        self.offsets, size = arena_layout(units, extra)
        self.arena = torch.zeros(size, device=self.device, dtype=torch.float32)

    def fill_conv(self, host, u, w, b):
        """Weight [Co, Ci, kh, kw] (or [Co, Ci] of a 1 x 1 unit) and bias of unit `u` into the host copy of the arena."""
        wo, bo = self.offsets[u.name]
        host[wo:wo + u.co * u.k] = w.detach().reshape(u.co, u.ci, u.kh, u.kw).permute(0, 2, 3, 1).reshape(-1).to(torch.float32)
        host[bo:bo + u.co] = b.detach().to(torch.float32)

    # ------------------------------------------------------------------ ops
    def new_map(self, B, H, W, C):
        return Map(torch.empty((B * H * W, C), device=self.device, dtype=torch.float32), B, H, W)

    def _out(self, out, B, H, W, C):
        """The map an op writes: a new one, the Map given, or the 2-D view given (a column slice of a wider buffer)."""
        y = self.new_map(B, H, W, C) if out is None else out if isinstance(out, Map) else Map(out, B, H, W)
        assert (y.B, y.H, y.W, y.C) == (B, H, W, C) and y.t.shape[0] == B * H * W, (y.B, y.H, y.W, y.C, tuple(y.t.shape))
        return y

    def conv(self, x, unit, relu, res=None, out=None):
        """One launch: the unit (a ConvUnit or its name) with its bias (+ res) (+ ReLU).  out may be res."""
        from .. import _pdmk as k
        u = unit if isinstance(unit, ConvUnit) else self.units[unit]
        assert x.C == u.ci, (u.name, x.C, u.ci)
        Ho, Wo = (x.H + 2 * u.ph - u.kh) // u.stride + 1, (x.W + 2 * u.pw - u.kw) // u.stride + 1
        if Ho < 1 or Wo < 1:
            raise ValueError(f"{type(self).__name__}: a {x.H} x {x.W} map is too small for {u.name}")
        y = self._out(out, x.B, Ho, Wo, u.co)
        wo, bo = self.offsets[u.name]
        w, b = self.arena[wo:wo + u.co * u.k], self.arena[bo:bo + u.co]
        if res is None:
            k.conv2d_fwd(x.t, x.ld, w, b, y.t, y.ld, x.B, x.H, x.W, u.ci, u.co, u.kh, u.kw, u.stride, u.ph, u.pw, relu=relu)
        else:
            assert (res.B, res.H, res.W, res.C) == (y.B, y.H, y.W, y.C), u.name
            k.conv2d_fwd_res(x.t, x.ld, w, b, res.t, res.ld, y.t, y.ld, x.B, x.H, x.W, u.ci, u.co, u.kh, u.kw, u.stride, u.ph,
                             u.pw, relu=relu)
        return y

    def pool(self, x, mode, stride, pad, out=None):
        """pdmk_pool2d: the 3 x 3 "max" / "avg" pool (the average divides by the taps inside the image)."""
        from .. import _pdmk as k
        Ho, Wo = (x.H + 2 * pad - 3) // stride + 1, (x.W + 2 * pad - 3) // stride + 1
        if Ho < 1 or Wo < 1:
            raise ValueError(f"{type(self).__name__}: a {x.H} x {x.W} map is too small for the 3 x 3 {mode} pool")
        y = self._out(out, x.B, Ho, Wo, x.C)
        k.pool2d(x.t, x.ld, y.t, y.ld, x.B, x.H, x.W, x.C, mode, stride, pad)
        return y
