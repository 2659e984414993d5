"""The unit table of torchvision's `resnet50` (ResNet v1.5: the stride of a downsampling bottleneck sits on its 3 x 3
`conv2`, not on `conv1`) under torchvision's key names.  Every unit is conv (no bias) -> BatchNorm(eps 1e-5); where the ReLU
goes is the forward pass's business (resnet50.py).  Pure Python: buildable without a GPU.  `build_units()` is ResNet-50 -
53 conv units + fc, 25 557 032 parameters; `build_units((1, 1, 1, 1))` is the four-bottleneck net of the tests.
"""
from dataclasses import dataclass

import torch

from ..inception.spec import fold_batchnorm as _fold

BN_EPS = 1e-5
NUM_CLASSES = 1000
WIDTHS = (64, 128, 256, 512)        # bottleneck width of layer1 .. layer4; the block's output is 4 x that
EXPANSION = 4


@dataclass(frozen=True)
class ConvUnit:
    conv: str       # state-dict key of the weight: <conv>.weight
    bn: str         # prefix of the BatchNorm: <bn>.{weight,bias,running_mean,running_var,num_batches_tracked}
    ci: int
    co: int
    kh: int = 1
    kw: int = 1
    stride: int = 1
    ph: int = 0
    pw: int = 0

    @property
    def name(self):
        return self.conv

    @property
    def k(self):
        return self.kh * self.kw * self.ci


def _u(conv, bn, ci, co, k=1, stride=1, pad=0):
    return ConvUnit(conv, bn, ci, co, k, k, stride, pad, pad)


def build_units(layers=(3, 4, 6, 3)):
    """The conv units in forward order: conv1, then per bottleneck conv1, conv2, conv3 and, in a layer's first block, the
    downsample conv behind them."""
    if len(layers) != 4 or min(layers) < 1:
        raise ValueError(f"layers: four positive block counts, got {layers}")
    units = [_u("conv1", "bn1", 3, 64, 7, 2, 3)]
    ci = 64
    for l, (n, wd) in enumerate(zip(layers, WIDTHS), start=1):
        for i in range(n):
            p, s = f"layer{l}.{i}", (2 if i == 0 and l > 1 else 1)
            units += [_u(f"{p}.conv1", f"{p}.bn1", ci, wd), _u(f"{p}.conv2", f"{p}.bn2", wd, wd, 3, s, 1),
                      _u(f"{p}.conv3", f"{p}.bn3", wd, wd * EXPANSION)]
            if i == 0:
                units.append(_u(f"{p}.downsample.0", f"{p}.downsample.1", ci, wd * EXPANSION, 1, s))
            ci = wd * EXPANSION
    return units


def fold_batchnorm(w, gamma, beta, mean, var):
    """inception.spec.fold_batchnorm (float64 on the host) with this network's eps."""
    return _fold(w, gamma, beta, mean, var, eps=BN_EPS)


def state_dict_shapes(units=None, num_batches_tracked=True):
    """{key: shape} in torchvision's naming, fc included."""
    out = {}
    for u in units or build_units():
        out[f"{u.conv}.weight"] = (u.co, u.ci, u.kh, u.kw)
        for s in ("weight", "bias", "running_mean", "running_var"):
            out[f"{u.bn}.{s}"] = (u.co,)
        if num_batches_tracked:
            out[f"{u.bn}.num_batches_tracked"] = ()
    out["fc.weight"] = (NUM_CLASSES, WIDTHS[-1] * EXPANSION)
    out["fc.bias"] = (NUM_CLASSES,)
    return out


def checked_trunk(sd, units=None):
    """The tensors the classifier uses: `num_batches_tracked` is ignored, a missing or mis-shaped key raises KeyError /
    ValueError naming it, any other key raises KeyError."""
    want = state_dict_shapes(units, num_batches_tracked=False)
    extra = [n for n in sd if n not in want and not n.endswith("num_batches_tracked")]
    if extra:
        raise KeyError(f"unexpected keys in the ResNet state dict: {sorted(extra)[:5]}")
    for n, shape in want.items():
        if n not in sd:
            raise KeyError(f"missing key {n} in the ResNet state dict")
        if tuple(sd[n].shape) != tuple(shape):
            raise ValueError(f"{n}: shape {tuple(sd[n].shape)}, expected {tuple(shape)}")
    return {n: sd[n] for n in want}


def init_state_dict(seed=0, units=None):
    """Seeded stand-in weights under torchvision's names (He-normal convs, BatchNorm scale 1 - 0.5 on each block's last
    BatchNorm so that 16 residual sums do not grow -, small random shift and running statistics, a small fc).  Tests
    calibrate the running statistics themselves; this is only a well-formed checkpoint."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for u in units or build_units():
        sd[f"{u.conv}.weight"] = torch.randn(u.co, u.ci, u.kh, u.kw, generator=g) * (2.0 / u.k) ** 0.5
        sd[f"{u.bn}.weight"] = torch.full((u.co,), 0.5 if u.bn.endswith("bn3") else 1.0)
        sd[f"{u.bn}.bias"] = torch.randn(u.co, generator=g) * 0.1
        sd[f"{u.bn}.running_mean"] = torch.randn(u.co, generator=g) * 0.1
        sd[f"{u.bn}.running_var"] = torch.rand(u.co, generator=g) * 0.5 + 0.75
        sd[f"{u.bn}.num_batches_tracked"] = torch.tensor(0)
    fan = WIDTHS[-1] * EXPANSION
    sd["fc.weight"] = torch.randn(NUM_CLASSES, fan, generator=g) * (1.0 / fan) ** 0.5
    sd["fc.bias"] = torch.randn(NUM_CLASSES, generator=g) * 0.1
    return sd
