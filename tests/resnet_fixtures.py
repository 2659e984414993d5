"""Fixtures of the object-erasure classifier tests: a functional plain-torch restatement of torchvision's ResNet-50 (v1.5, the
stride on the 3 x 3 conv2) with UNFOLDED BatchNorm, written out without pdm/models/resnet/spec.py; seeded weights whose
BatchNorm running statistics are calibrated on the fixture images (as fid_fixtures.calibrated_state_dict does), so that
activations neither die nor blow up over 16 residual blocks; the preset's preprocessing with PIL; and softmax / top-k under
this project's tie rule.  Everything runs in float64 (the oracle) and in float32 (the yardstick: its distance from float64
sizes the tolerances).

Two fixture conditions are asserted on the CPU before anything is compared (`check_logits`, `check_gaps`): the float32
restatement's logits lie within 1e-4 of the logit range of float64's, and the float64 top-(k + 1) probabilities are at least
100 x the float32 restatement's probability error apart - index comparisons are then exact, with no case left out."""
import numpy as np
import torch
import torch.nn.functional as F

import fid_fixtures as ffx

EPS = 1e-5
WIDTHS = (64, 128, 256, 512)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TINY, FULL = (1, 1, 1, 1), (3, 4, 6, 3)


def image(seed, h, w):
    return ffx.structured_image(seed, h, w)


def normalised(img_u8):
    """ToTensor + Normalize in float32 (the preset's arithmetic): [1, 3, H, W]."""
    x = np.asarray(img_u8, np.uint8).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    x = (x - np.asarray(MEAN, np.float32).reshape(3, 1, 1)) / np.asarray(STD, np.float32).reshape(3, 1, 1)
    return torch.from_numpy(x)[None]


def preset(img_u8, resize_size, crop_size):
    """torchvision's ImageClassification preset on a PIL image: bilinear resize of the short side (long side
    int(size * long / short)), centre crop at int(round((side - crop) / 2.0)), ToTensor, Normalize -> float32 [1, 3, R, R]."""
    from PIL import Image
    h, w = img_u8.shape[:2]
    rh, rw = (int(resize_size * h / w), resize_size) if w <= h else (resize_size, int(resize_size * w / h))
    im = Image.fromarray(img_u8, "RGB")
    if (rh, rw) != (h, w):
        im = im.resize((rw, rh), Image.BILINEAR)
    top, left = int(round((rh - crop_size) / 2.0)), int(round((rw - crop_size) / 2.0))
    return normalised(np.asarray(im.crop((left, top, left + crop_size, top + crop_size)), np.uint8))


def block_names(layers):
    """[(prefix, width, stride, has_downsample)] in forward order."""
    out = []
    for l, (n, wd) in enumerate(zip(layers, WIDTHS), start=1):
        for i in range(n):
            out.append((f"layer{l}.{i}", wd, 2 if (i == 0 and l > 1) else 1, i == 0))
    return out


class Net:
    """ResNet over a state dict with torchvision's keys.  calibrate=True: every BatchNorm first takes its running statistics
    from the batch passing through (mean and biased variance)."""

    def __init__(self, sd, layers, calibrate=False):
        self.sd, self.layers, self.calibrate = sd, layers, calibrate

    def cbn(self, x, conv, bn, stride=1, padding=0):
        sd = self.sd
        x = F.conv2d(x, sd[conv + ".weight"].to(x.dtype), None, stride, padding)
        if self.calibrate:
            sd[bn + ".running_mean"] = x.mean((0, 2, 3)).to(torch.float32)
            sd[bn + ".running_var"] = x.var((0, 2, 3), unbiased=False).to(torch.float32)
        return F.batch_norm(x, sd[bn + ".running_mean"].to(x.dtype), sd[bn + ".running_var"].to(x.dtype),
                            sd[bn + ".weight"].to(x.dtype), sd[bn + ".bias"].to(x.dtype), False, 0.0, EPS)

    def __call__(self, x):
        """x [B, 3, H, W] normalised -> logits [B, 1000]."""
        x = F.relu(self.cbn(x, "conv1", "bn1", 2, 3))
        x = F.max_pool2d(x, 3, 2, 1)
        for p, wd, s, down in block_names(self.layers):
            t = F.relu(self.cbn(x, p + ".conv1", p + ".bn1"))
            t = F.relu(self.cbn(t, p + ".conv2", p + ".bn2", s, 1))
            t = self.cbn(t, p + ".conv3", p + ".bn3")
            if down:
                x = self.cbn(x, p + ".downsample.0", p + ".downsample.1", s)
            x = F.relu(t + x)
        x = F.adaptive_avg_pool2d(x, 1).flatten(1)
        return F.linear(x, self.sd["fc.weight"].to(x.dtype), self.sd["fc.bias"].to(x.dtype))


def seeded_state_dict(layers, seed=0):
    """He-normal convs, BatchNorm weight 1 (0.5 on a block's last BatchNorm) / small seeded bias, running statistics to be
    calibrated, an fc with unit-variance logits."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def unit(conv, bn, ci, co, k, gamma=1.0):
        sd[conv + ".weight"] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[bn + ".weight"] = torch.full((co,), gamma)
        sd[bn + ".bias"] = torch.randn(co, generator=g) * 0.2
        sd[bn + ".running_mean"] = torch.zeros(co)
        sd[bn + ".running_var"] = torch.ones(co)
        sd[bn + ".num_batches_tracked"] = torch.tensor(0)

    unit("conv1", "bn1", 3, 64, 7)
    ci = 64
    for p, wd, s, down in block_names(layers):
        unit(p + ".conv1", p + ".bn1", ci, wd, 1)
        unit(p + ".conv2", p + ".bn2", wd, wd, 3)
        unit(p + ".conv3", p + ".bn3", wd, 4 * wd, 1, 0.5)
        if down:
            unit(p + ".downsample.0", p + ".downsample.1", ci, 4 * wd, 1)
        ci = 4 * wd
    sd["fc.weight"] = torch.randn(1000, 2048, generator=g) * (4.0 / 2048) ** 0.5
    sd["fc.bias"] = torch.randn(1000, generator=g) * 0.5
    return sd


_CACHE = {}


@torch.no_grad()
def calibrated_state_dict(layers, seed=0, n_calib=16):
    """seeded_state_dict with the running statistics of one calibration pass (float32) over n_calib structured 64 x 64
    images."""
    key = (tuple(layers), seed, n_calib)
    if key not in _CACHE:
        sd = seeded_state_dict(layers, seed)
        x = torch.cat([normalised(image(900 + i, 64, 64)) for i in range(n_calib)])
        Net(sd, layers, calibrate=True)(x)
        _CACHE[key] = sd
    return dict(_CACHE[key])


@torch.no_grad()
def oracle_logits(sd, layers, x32, dtype):
    """Logits [B, 1000] (float64 numpy) of the float32 input batch evaluated in `dtype`."""
    return Net(sd, layers)(x32.to(dtype)).to(torch.float64).numpy()


def softmax_topk(logits, k):
    """(probs [B, k], idx [B, k]) of float64 softmax rows under the project's rule: larger first, ties lower index first, a
    NaN above everything (lower index first among NaNs)."""
    z = np.asarray(logits, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(np.isnan(z), -np.inf, z).max(axis=1, keepdims=True)
        e = np.exp(z - m)
        p = e / e.sum(axis=1, keepdims=True)
    nan = np.isnan(z)
    rank = np.where(nan, 0.0, z)
    idx = np.stack([np.lexsort((np.arange(z.shape[1]), -r, ~n))[:k] for r, n in zip(rank, nan)])     # last key first
    return np.take_along_axis(p, idx, 1), idx


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def check_logits(ref64, cpu32, what):
    """Fixture condition 1: float32 restatement logits within 1e-4 of the logit range of float64's."""
    rng = float(ref64.max() - ref64.min())
    err = float(np.abs(cpu32 - ref64).max())
    print(f"{what}: fixture logits fp32 err / range {err / rng:.3e}")
    assert err <= 1e-4 * rng, f"fixture: {what} float32 logits are {err / rng:.3e} of the range off float64"


def check_gaps(ref64_logits, cpu32_logits, k, what):
    """Fixture condition 2: in float64 the gaps between consecutive top-(k + 1) probabilities (top-N where N == k) are at
    least 100 x the float32 restatement's probability error.  Returns (float64 probs, idx, float32 probs) of the top k."""
    n = ref64_logits.shape[1]
    p64, i64 = softmax_topk(ref64_logits, min(k + 1, n))
    with np.errstate(over="ignore"):
        z = np.asarray(cpu32_logits, np.float32)
        e = np.exp(z - z.max(axis=1, keepdims=True), dtype=np.float32)
        p32_all = (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float64)
    p32 = np.take_along_axis(p32_all, i64, 1)
    err = float(np.abs(p32 - p64).max())
    if p64.shape[1] > 1:
        gap = float((p64[:, :-1] - p64[:, 1:]).min())
        print(f"{what}: fixture min top-{p64.shape[1]} gap {gap:.3e}, fp32 prob err {err:.3e}")
        assert gap >= 100 * err, f"fixture: {what} gap {gap:.3e} is below 100 x the float32 probability error {err:.3e}"
    return p64[:, :k], i64[:, :k], p32[:, :k]


def yardstick(ref64, cpu32, got, what):
    """The project's yardstick for ONE quantity over a batch: scale = max |ref64|; max |got - ref64| may be at most 8 x
    max |cpu32 - ref64|, floor 8 fp32 ulps of the scale.  Prints the figures; returns the failures (empty: passed)."""
    r, c, g = (np.asarray(np.ravel(v), np.float64) for v in (ref64, cpu32, got))
    assert r.shape == c.shape == g.shape and r.size, (r.shape, c.shape, g.shape)
    scale = np.abs(r).max()
    yard = max(8 * np.abs(c - r).max(), 8 * ulp32(scale))
    err = np.abs(g - r).max()
    print(f"{what}: err/max {err / scale:.3e}, yardstick/max {yard / scale:.3e}")
    return [] if err <= yard else [(what, err, yard)]
