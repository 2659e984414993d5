"""Layer tables of the two trunks of the perceptual metrics, under the upstream key names.  Pure Python: no GPU needed.

* AlexNet (torchvision `alexnet().features`, the `net='alex'` trunk of lpips v0.1): features.{0,3,6,8,10}, every conv followed
  by a ReLU, a 3 x 3 stride-2 max pool behind the first two; the five post-ReLU maps are LPIPS' taps.  The linear heads are
  lpips' `lin{0..4}.model.1.weight` [1, C, 1, 1] (weights/v0.1/alex.pth).
* VGG-19 (torchvision `vgg19().features`): features.{0,2,5,7,10}, 3 x 3 / pad 1, a 2 x 2 max pool behind conv_2 and conv_4;
  the reference's styleloss.py trims everything behind conv_5.  Its taps are the PRE-ReLU conv outputs.
"""
import torch

from ..convnet import ConvUnit

ALEX_UNITS = (ConvUnit("features.0", 3, 64, 11, 11, 4, 2, 2), ConvUnit("features.3", 64, 192, 5, 5, 1, 2, 2),
              ConvUnit("features.6", 192, 384, 3, 3, 1, 1, 1), ConvUnit("features.8", 384, 256, 3, 3, 1, 1, 1),
              ConvUnit("features.10", 256, 256, 3, 3, 1, 1, 1))
ALEX_POOL_AFTER = (0, 1)                      # 0-based conv index followed by MaxPool2d(3, 2)
LPIPS_CHANNELS = tuple(u.co for u in ALEX_UNITS)
LPIPS_SHIFT = (-0.030, -0.088, -0.188)        # lpips.ScalingLayer, applied to the [-1, 1] image
LPIPS_SCALE = (0.458, 0.448, 0.450)

VGG_UNITS = (ConvUnit("features.0", 3, 64, 3, 3, 1, 1, 1), ConvUnit("features.2", 64, 64, 3, 3, 1, 1, 1),
             ConvUnit("features.5", 64, 128, 3, 3, 1, 1, 1), ConvUnit("features.7", 128, 128, 3, 3, 1, 1, 1),
             ConvUnit("features.10", 128, 256, 3, 3, 1, 1, 1))
VGG_POOL_AFTER = (1, 3)                       # conv_2 and conv_4 are followed by ReLU + MaxPool2d(2, 2)
VGG_CONTENT = 3                               # conv_4
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
STYLE_WEIGHT, CONTENT_WEIGHT = 1000000, 1     # styleloss.py get_style_content_loss

ALEX_WEIGHTS_NAME = "alexnet-owt-7be5be79.pth"
VGG_WEIGHTS_NAME = "vgg19-dcbb9e9d.pth"
LPIPS_WEIGHTS_NAME = "alex.pth"


def lin_key(i):
    return f"lin{i}.model.1.weight"


def lpips_input_norm():
    """(mean, std) of the [0, 1] image that equal the ScalingLayer of the [-1, 1] image: ((2 x - 1) - shift) / scale."""
    return tuple(0.5 + 0.5 * s for s in LPIPS_SHIFT), tuple(0.5 * s for s in LPIPS_SCALE)


def conv_shapes(units):
    out = {}
    for u in units:
        out[f"{u.name}.weight"] = (u.co, u.ci, u.kh, u.kw)
        out[f"{u.name}.bias"] = (u.co,)
    return out


def lin_shapes():
    return {lin_key(i): (1, c, 1, 1) for i, c in enumerate(LPIPS_CHANNELS)}


def init_conv_state_dict(units, seed):
    """Seeded stand-in weights (He-normal, small biases) under the upstream names: a well-formed checkpoint, not a trained one."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for u in units:
        sd[f"{u.name}.weight"] = torch.randn(u.co, u.ci, u.kh, u.kw, generator=g) * (2.0 / u.k) ** 0.5
        sd[f"{u.name}.bias"] = torch.randn(u.co, generator=g) * 0.1
    return sd


def init_lin_state_dict(seed):
    g = torch.Generator().manual_seed(seed)
    return {lin_key(i): torch.rand(1, c, 1, 1, generator=g) for i, c in enumerate(LPIPS_CHANNELS)}
