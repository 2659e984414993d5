"""Fixtures of the FID tests: a plain-torch CPU restatement of clean-fid's `legacy_pytorch` pipeline up to the features
(bilinear resize to 299 x 299 without antialiasing -> pytorch-fid's InceptionV3 pool3), written out unit by unit in
torchvision's forward order and independent of pdm/models/inception/spec.py; seeded weights whose BatchNorm running
statistics are calibrated on images, and structured seeded images.  The restatement runs in float64 (the oracle) and in
float32 (the yardstick: its own error against float64 sizes the tolerances)."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3


def structured_image(seed, h, w, family=0):
    """uint8 [h, w, 3]: low-resolution colour blobs upsampled smoothly, plus noise.  family 1: finer, darker, red-tinted blobs
    (a second distribution for the end-to-end FID)."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = (3, 9) if family == 0 else (8, 17)
    gh, gw = int(torch.randint(lo, hi, (1,), generator=g)), int(torch.randint(lo, hi, (1,), generator=g))
    low = torch.rand(1, 3, gh, gw, generator=g)
    if family:
        low = low * torch.tensor([0.9, 0.5, 0.6]).reshape(1, 3, 1, 1)
    img = F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0]
    img = img * 255 + torch.randn(3, h, w, generator=g) * 12
    return img.clamp(0, 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


SIZES = [(512, 512), (427, 640), (299, 299), (256, 384), (330, 300), (600, 450), (128, 128), (300, 500)]


def images(seed, n, sizes=SIZES, family=0):
    return [structured_image(seed * 1000 + i, *sizes[i % len(sizes)], family=family) for i in range(n)]


def resize_input(img_u8, dtype=torch.float32):
    """Items 2-3: the uint8 image as float32 in 0..255, bilinear to 299 x 299 (no antialiasing), clip - float32 whatever
    `dtype` is: that IS the specification (a float64 resize forms its source coordinates differently by up to 6e-5 of a pixel
    step, which would be charged to the network's round-off) - then / 255 in `dtype`.  [1, 3, 299, 299]."""
    x = torch.from_numpy(np.ascontiguousarray(img_u8)).permute(2, 0, 1)[None].to(torch.float32)
    x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False).clamp(0, 255)
    return x.to(dtype) / 255


class Net:
    """The FID Inception over a state dict with pytorch-fid's keys.  calibrate=True: every BatchNorm first takes its running
    statistics from the batch passing through (mean and biased variance), as one training-mode pass with momentum 1 would."""

    def __init__(self, sd, calibrate=False):
        self.sd, self.calibrate = sd, calibrate

    def unit(self, x, name, stride=1, padding=0):
        sd = self.sd
        x = F.conv2d(x, sd[name + ".conv.weight"].to(x.dtype), None, stride, padding)
        if self.calibrate:
            sd[name + ".bn.running_mean"] = x.mean((0, 2, 3)).to(torch.float32)
            sd[name + ".bn.running_var"] = x.var((0, 2, 3), unbiased=False).to(torch.float32)
        x = F.batch_norm(x, sd[name + ".bn.running_mean"].to(x.dtype), sd[name + ".bn.running_var"].to(x.dtype),
                         sd[name + ".bn.weight"].to(x.dtype), sd[name + ".bn.bias"].to(x.dtype), False, 0.0, EPS)
        return F.relu(x)

    def block_a(self, x, n):
        u = self.unit
        b1 = u(x, n + ".branch1x1")
        b5 = u(u(x, n + ".branch5x5_1"), n + ".branch5x5_2", padding=2)
        b3 = u(u(u(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2", padding=1), n + ".branch3x3dbl_3", padding=1)
        bp = u(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), n + ".branch_pool")
        return torch.cat([b1, b5, b3, bp], 1)

    def block_b(self, x, n):
        u = self.unit
        b3 = u(x, n + ".branch3x3", stride=2)
        bd = u(u(u(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2", padding=1), n + ".branch3x3dbl_3", stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)

    def block_c(self, x, n):
        u = self.unit
        b1 = u(x, n + ".branch1x1")
        b7 = u(u(u(x, n + ".branch7x7_1"), n + ".branch7x7_2", padding=(0, 3)), n + ".branch7x7_3", padding=(3, 0))
        bd = u(x, n + ".branch7x7dbl_1")
        bd = u(u(bd, n + ".branch7x7dbl_2", padding=(3, 0)), n + ".branch7x7dbl_3", padding=(0, 3))
        bd = u(u(bd, n + ".branch7x7dbl_4", padding=(3, 0)), n + ".branch7x7dbl_5", padding=(0, 3))
        bp = u(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), n + ".branch_pool")
        return torch.cat([b1, b7, bd, bp], 1)

    def block_d(self, x, n):
        u = self.unit
        b3 = u(u(x, n + ".branch3x3_1"), n + ".branch3x3_2", stride=2)
        b7 = u(u(u(x, n + ".branch7x7x3_1"), n + ".branch7x7x3_2", padding=(0, 3)), n + ".branch7x7x3_3", padding=(3, 0))
        b7 = u(b7, n + ".branch7x7x3_4", stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)

    def block_e(self, x, n, pool):
        u = self.unit
        b1 = u(x, n + ".branch1x1")
        b3 = u(x, n + ".branch3x3_1")
        b3 = torch.cat([u(b3, n + ".branch3x3_2a", padding=(0, 1)), u(b3, n + ".branch3x3_2b", padding=(1, 0))], 1)
        bd = u(u(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2", padding=1)
        bd = torch.cat([u(bd, n + ".branch3x3dbl_3a", padding=(0, 1)), u(bd, n + ".branch3x3dbl_3b", padding=(1, 0))], 1)
        p = F.avg_pool2d(x, 3, 1, 1, count_include_pad=False) if pool == "avg" else F.max_pool2d(x, 3, 1, 1)
        return torch.cat([b1, b3, bd, u(p, n + ".branch_pool")], 1)

    def __call__(self, x01):
        """x01 [B, 3, 299, 299] in [0, 1] -> [B, 2048]."""
        u = self.unit
        x = 2 * x01 - 1
        x = u(u(u(x, "Conv2d_1a_3x3", stride=2), "Conv2d_2a_3x3"), "Conv2d_2b_3x3", padding=1)
        x = F.max_pool2d(x, 3, 2)
        x = u(u(x, "Conv2d_3b_1x1"), "Conv2d_4a_3x3")
        x = F.max_pool2d(x, 3, 2)
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = self.block_a(x, n)
        x = self.block_b(x, "Mixed_6a")
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self.block_c(x, n)
        x = self.block_d(x, "Mixed_7a")
        x = self.block_e(x, "Mixed_7b", "avg")
        x = self.block_e(x, "Mixed_7c", "max")
        return F.adaptive_avg_pool2d(x, 1).flatten(1)


def seeded_state_dict(seed=0):
    """He-normal convs, BatchNorm weight 1 / small seeded bias, 1008-way fc (unused) - under pytorch-fid's key names, the
    running statistics to be calibrated."""
    from pdm.models.inception.spec import state_dict_shapes
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in state_dict_shapes().items():
        if name.endswith("conv.weight"):
            sd[name] = torch.randn(*shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif name.endswith("bn.weight"):
            sd[name] = torch.ones(shape)
        elif name.endswith("bn.bias"):
            sd[name] = torch.randn(*shape, generator=g) * 0.2
        elif name.endswith("running_mean"):
            sd[name] = torch.zeros(shape)
        elif name.endswith("running_var"):
            sd[name] = torch.ones(shape)
        else:
            sd[name] = torch.tensor(0)
    sd["fc.weight"] = torch.randn(1008, 2048, generator=g) * 0.01
    sd["fc.bias"] = torch.zeros(1008)
    return sd


_CACHE = {}


@torch.no_grad()
def calibrated_state_dict(seed=0, n_calib=16):
    """seeded_state_dict with the running statistics of one calibration pass over n_calib structured images (float32)."""
    key = (seed, n_calib)
    if key not in _CACHE:
        sd = seeded_state_dict(seed)
        x = torch.cat([resize_input(im) for im in images(7, n_calib)])
        Net(sd, calibrate=True)(x)
        _CACHE[key] = sd
    return dict(_CACHE[key])


@torch.no_grad()
def oracle_features(sd, imgs, dtype, chunk=16):
    """Features [N, 2048] of the uint8 images through the restatement in `dtype` (float64 numpy out)."""
    net = Net(sd)
    out = []
    for i in range(0, len(imgs), chunk):
        x = torch.cat([resize_input(im, dtype) for im in imgs[i:i + chunk]])
        out.append(net(x).to(torch.float64))
    return torch.cat(out).numpy()


def stats(feats):
    f = np.asarray(feats, np.float64)
    return f.mean(axis=0), np.cov(f, rowvar=False)
