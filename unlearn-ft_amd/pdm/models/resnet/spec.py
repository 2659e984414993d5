"""The unit table of torchvision's `resnet50` (ResNet v1.5: the stride of a downsampling bottleneck sits on its 3 x 3
`conv2`, not on `conv1`) under torchvision's key names.  Every unit is conv (no bias) -> BatchNorm(eps 1e-5); where the ReLU
goes is the forward pass's business (resnet50.py).  Pure Python: buildable without a GPU.  `build_units()` is ResNet-50 -
53 conv units + fc, 25 557 032 parameters; `build_units((1, 1, 1, 1))` is the four-bottleneck net of the tests.
"""
import torch

from ..convnet import ConvUnit, conv_bn_shapes

BN_EPS = 1e-5
NUM_CLASSES = 1000
WIDTHS = (64, 128, 256, 512)        # bottleneck width of layer1 .. layer4; the block's output is 4 x that
EXPANSION = 4
FC = ConvUnit("fc", WIDTHS[-1] * EXPANSION, NUM_CLASSES)        # the classifier: a 1 x 1 unit on the pooled [B, 2048] map


def keys(u):
    """(conv prefix, BatchNorm prefix) of a unit, its name being the conv's: conv1 -> bn1, layerL.I.convN -> layerL.I.bnN,
    layerL.I.downsample.0 -> layerL.I.downsample.1."""
    return u.name, (u.name[:-1] + "1" if u.name.endswith("downsample.0") else u.name.replace("conv", "bn"))


def _u(name, ci, co, k=1, stride=1, pad=0):
    return ConvUnit(name, ci, co, k, k, stride, pad, pad)


def build_units(layers=(3, 4, 6, 3)):
    """The conv units in forward order: conv1, then per bottleneck conv1, conv2, conv3 and, in a layer's first block, the
    downsample conv behind them."""
    if len(layers) != 4 or min(layers) < 1:
        raise ValueError(f"layers: four positive block counts, got {layers}")
    units = [_u("conv1", 3, 64, 7, 2, 3)]
    ci = 64
    for l, (n, wd) in enumerate(zip(layers, WIDTHS), start=1):
        for i in range(n):
            p, s = f"layer{l}.{i}", (2 if i == 0 and l > 1 else 1)
            units += [_u(f"{p}.conv1", ci, wd), _u(f"{p}.conv2", wd, wd, 3, s, 1), _u(f"{p}.conv3", wd, wd * EXPANSION)]
            if i == 0:
                units.append(_u(f"{p}.downsample.0", ci, wd * EXPANSION, 1, s))
            ci = wd * EXPANSION
    return units


def state_dict_shapes(units=None, num_batches_tracked=True):
    """{key: shape} in torchvision's naming, fc included."""
    out = conv_bn_shapes(units or build_units(), keys, num_batches_tracked)
    out["fc.weight"] = (FC.co, FC.ci)
    out["fc.bias"] = (FC.co,)
    return out


def ignored(key):
    """The keys of a torchvision state dict that the classifier does not use (convnet.checked raises on any other stray)."""
    return key.endswith("num_batches_tracked")


def init_state_dict(seed=0, units=None):
    """Seeded stand-in weights under torchvision's names (He-normal convs, BatchNorm scale 1 - 0.5 on each block's last
    BatchNorm so that 16 residual sums do not grow -, small random shift and running statistics, a small fc).  Tests
    calibrate the running statistics themselves; this is only a well-formed checkpoint."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for u in units or build_units():
        conv, bn = keys(u)
        sd[f"{conv}.weight"] = torch.randn(u.co, u.ci, u.kh, u.kw, generator=g) * (2.0 / u.k) ** 0.5
        sd[f"{bn}.weight"] = torch.full((u.co,), 0.5 if bn.endswith("bn3") else 1.0)
        sd[f"{bn}.bias"] = torch.randn(u.co, generator=g) * 0.1
        sd[f"{bn}.running_mean"] = torch.randn(u.co, generator=g) * 0.1
        sd[f"{bn}.running_var"] = torch.rand(u.co, generator=g) * 0.5 + 0.75
        sd[f"{bn}.num_batches_tracked"] = torch.tensor(0)
    sd["fc.weight"] = torch.randn(FC.co, FC.ci, generator=g) * (1.0 / FC.ci) ** 0.5
    sd["fc.bias"] = torch.randn(FC.co, generator=g) * 0.1
    return sd
