"""`InceptionV3FID`: pytorch-fid's `InceptionV3(output_blocks=[3])` on libpdmk - the feature extractor of clean-fid's
`legacy_pytorch` FID (pdm/utils/fid_utils.py).  fp32, inference only, NHWC.

Every unit is one pdmk_conv2d_fwd launch (implicit GEMM on exact-fp32 MFMA, BatchNorm folded into weight and bias in
float64 on the host, ReLU in the epilogue); the 1x1 units go through the same kernel, so they get the fused ReLU and the
column-slice output too.  A Mixed block allocates its output [B * H * W, C_out] once and every branch's last unit writes
its column slice of it (row stride C_out): no concat copies.  Pools are pdmk_pool2d (the branch_pool average divides by
the taps inside the image; Mixed_7c's branch_pool is a max pool - the FID network's deviations from torchvision's), the
head is pdmk_global_avgpool over the 8 x 8 map.  Launches are eager on the current stream.
"""
import os

import torch

from ... import _pdmk as k
from .spec import build_units, checked_trunk, fold_batchnorm, init_state_dict

WEIGHTS_NAME = "pt_inception-2015-12-05-6726825d.pth"
INPUT_SIZE = 299
FEATURE_DIM = 2048


def default_weights_path():
    """Where torch hub keeps pytorch-fid's / clean-fid's Inception weights."""
    return os.path.join(os.path.expanduser("~"), ".cache", "torch", "hub", "checkpoints", WEIGHTS_NAME)


class _Map:
    """An NHWC activation: t is a 2-D view [B * H * W, C] of a buffer whose row stride may be wider than C."""

    def __init__(self, t, B, H, W):
        self.t, self.B, self.H, self.W, self.C, self.ld = t, B, H, W, t.shape[1], t.stride(0)


class InceptionV3FID:
    def __init__(self, device=None, seed=0, init=True):
        if not torch.cuda.is_available():
            raise RuntimeError("InceptionV3FID (MI355X engine) needs a GPU; there is no CPU fallback")
        self.device = torch.device(device or "cuda:0")
        self.units = {u.name: u for u in build_units()}
        off, self.offsets = 0, {}
        for u in self.units.values():                       # weight [Co, kh * kw * Ci] then bias [Co], each on a 512-byte line
            self.offsets[u.name] = (off, off + (u.co * u.k + 127) // 128 * 128)
            off = self.offsets[u.name][1] + (u.co + 127) // 128 * 128
        self.arena = torch.zeros(off, device=self.device, dtype=torch.float32)
        if init:
            self.load_state_dict(init_state_dict(seed))

    @classmethod
    def from_pretrained(cls, path=None, device=None):
        """The weights file given, else torch hub's cache; never fetched."""
        path = path or default_weights_path()
        if not os.path.isfile(path):
            raise FileNotFoundError(f"Inception weights not found at {path}: place pytorch-fid's {WEIGHTS_NAME} there or pass "
                                    f"--inception_weights FILE (nothing is downloaded)")
        sd = torch.load(path, map_location="cpu", weights_only=True)
        model = cls(device=device, init=False)
        model.load_state_dict(sd)
        return model

    def load_state_dict(self, sd):
        """pytorch-fid's keys; fc.*, AuxLogits.* and num_batches_tracked are ignored, a missing / mis-shaped trunk key raises."""
        sd = checked_trunk(sd, list(self.units.values()))
        host = torch.zeros(self.arena.numel(), dtype=torch.float32)
        for u in self.units.values():
            n = u.name
            w, b = fold_batchnorm(sd[f"{n}.conv.weight"], sd[f"{n}.bn.weight"], sd[f"{n}.bn.bias"], sd[f"{n}.bn.running_mean"],
                                  sd[f"{n}.bn.running_var"])
            wo, bo = self.offsets[n]
            host[wo:wo + u.co * u.k] = w.permute(0, 2, 3, 1).reshape(-1).to(torch.float32)       # k = (ky, kx, ci)
            host[bo:bo + u.co] = b.to(torch.float32)
        self.arena.copy_(host)

    # ------------------------------------------------------------------ ops
    def _new(self, B, H, W, C):
        return _Map(torch.empty((B * H * W, C), device=self.device, dtype=torch.float32), B, H, W)

    def conv(self, x, name, out=None):
        u = self.units[name]
        assert x.C == u.ci, (name, x.C, u.ci)
        Ho, Wo = (x.H + 2 * u.ph - u.kh) // u.stride + 1, (x.W + 2 * u.pw - u.kw) // u.stride + 1
        y = _Map(out, x.B, Ho, Wo) if out is not None else self._new(x.B, Ho, Wo, u.co)
        assert y.C == u.co and y.t.shape[0] == x.B * Ho * Wo
        wo, bo = self.offsets[name]
        k.conv2d_fwd(x.t, x.ld, self.arena[wo:wo + u.co * u.k], self.arena[bo:bo + u.co], y.t, y.ld, x.B, x.H, x.W, u.ci, u.co,
                     u.kh, u.kw, u.stride, u.ph, u.pw, relu=True)
        return y

    def pool(self, x, mode, stride, pad, out=None):
        Ho, Wo = (x.H + 2 * pad - 3) // stride + 1, (x.W + 2 * pad - 3) // stride + 1
        y = _Map(out, x.B, Ho, Wo) if out is not None else self._new(x.B, Ho, Wo, x.C)
        k.pool2d(x.t, x.ld, y.t, y.ld, x.B, x.H, x.W, x.C, mode, stride, pad)
        return y

    def _chain(self, x, names, out):
        for n in names[:-1]:
            x = self.conv(x, n)
        return self.conv(x, names[-1], out=out)

    def _mixed(self, x, n, widths, stride=1):
        """The block's output map and its column slices, one per entry of `widths`."""
        H, W = ((x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1) if stride == 2 else (x.H, x.W)
        y = self._new(x.B, H, W, sum(widths))
        cols, c = [], 0
        for wd in widths:
            cols.append(y.t[:, c:c + wd])
            c += wd
        return y, cols

    def _block_a(self, x, n):
        y, s = self._mixed(x, n, [64, 64, 96, self.units[f"{n}.branch_pool"].co])
        self.conv(x, f"{n}.branch1x1", out=s[0])
        self._chain(x, [f"{n}.branch5x5_1", f"{n}.branch5x5_2"], s[1])
        self._chain(x, [f"{n}.branch3x3dbl_1", f"{n}.branch3x3dbl_2", f"{n}.branch3x3dbl_3"], s[2])
        self.conv(self.pool(x, "avg", 1, 1), f"{n}.branch_pool", out=s[3])
        return y

    def _block_b(self, x, n):
        y, s = self._mixed(x, n, [384, 96, x.C], stride=2)
        self.conv(x, f"{n}.branch3x3", out=s[0])
        self._chain(x, [f"{n}.branch3x3dbl_1", f"{n}.branch3x3dbl_2", f"{n}.branch3x3dbl_3"], s[1])
        self.pool(x, "max", 2, 0, out=s[2])
        return y

    def _block_c(self, x, n):
        y, s = self._mixed(x, n, [192, 192, 192, 192])
        self.conv(x, f"{n}.branch1x1", out=s[0])
        self._chain(x, [f"{n}.branch7x7_{i}" for i in (1, 2, 3)], s[1])
        self._chain(x, [f"{n}.branch7x7dbl_{i}" for i in (1, 2, 3, 4, 5)], s[2])
        self.conv(self.pool(x, "avg", 1, 1), f"{n}.branch_pool", out=s[3])
        return y

    def _block_d(self, x, n):
        y, s = self._mixed(x, n, [320, 192, x.C], stride=2)
        self._chain(x, [f"{n}.branch3x3_1", f"{n}.branch3x3_2"], s[0])
        self._chain(x, [f"{n}.branch7x7x3_{i}" for i in (1, 2, 3, 4)], s[1])
        self.pool(x, "max", 2, 0, out=s[2])
        return y

    def _block_e(self, x, n, pool):
        y, s = self._mixed(x, n, [320, 384, 384, 384, 384, 192])
        self.conv(x, f"{n}.branch1x1", out=s[0])
        b = self.conv(x, f"{n}.branch3x3_1")
        self.conv(b, f"{n}.branch3x3_2a", out=s[1])
        self.conv(b, f"{n}.branch3x3_2b", out=s[2])
        b = self.conv(self.conv(x, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2")
        self.conv(b, f"{n}.branch3x3dbl_3a", out=s[3])
        self.conv(b, f"{n}.branch3x3dbl_3b", out=s[4])
        self.conv(self.pool(x, pool, 1, 1), f"{n}.branch_pool", out=s[5])
        return y

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward_nhwc(self, x):
        """x fp32 [B, 299, 299, 3] in [-1, 1] on the device -> pool3 features [B, 2048] fp32."""
        B, H, W, C = x.shape
        assert C == 3 and x.dtype == torch.float32 and x.is_contiguous() and min(H, W) >= 75, tuple(x.shape)
        m = _Map(x.reshape(B * H * W, 3), B, H, W)
        for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            m = self.conv(m, n)
        m = self.pool(m, "max", 2, 0)
        m = self.conv(self.conv(m, "Conv2d_3b_1x1"), "Conv2d_4a_3x3")
        m = self.pool(m, "max", 2, 0)
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            m = self._block_a(m, n)
        m = self._block_b(m, "Mixed_6a")
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            m = self._block_c(m, n)
        m = self._block_d(m, "Mixed_7a")
        m = self._block_e(m, "Mixed_7b", "avg")
        m = self._block_e(m, "Mixed_7c", "max")
        out = torch.empty((B, m.C), device=self.device, dtype=torch.float32)
        k.global_avgpool(m.t, m.ld, out, B, m.H * m.W, m.C)
        return out

    @torch.no_grad()
    def features(self, images):
        """uint8 images -> [B, 2048] fp32: a list of [H, W, 3] arrays / tensors (any sizes) or one [B, H, W, 3] tensor,
        resized on the device (pdmk_resize_bilinear_u8) and run through the network."""
        from ...utils.fid_utils import pack_images, prep_images
        if torch.is_tensor(images) and images.dim() == 4:
            images = list(images.cpu())
        arrays = [torch.as_tensor(a).cpu().numpy() for a in images]
        packed, desc = pack_images(arrays)
        return self.forward_nhwc(prep_images(packed, desc, self.device))
