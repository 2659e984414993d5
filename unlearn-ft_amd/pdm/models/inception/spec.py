"""The unit table of pytorch-fid's `InceptionV3(output_blocks=[3])` (the FID network; clean-fid's `legacy_pytorch` mode): the
trunk of torchvision's `inception_v3` under torchvision's key names, every unit conv (no bias) -> BatchNorm(eps 1e-3) -> ReLU.
Pure Python: buildable without a GPU.  94 units, 21 785 568 trunk parameters, 564 state-dict entries.

The three deviations of the FID network from torchvision's are in the forward pass (inception_v3.py), not in the table: the
branch_pool average of Mixed_5b/5c/5d, 6b-6e and 7b divides by the number of taps inside the image, Mixed_7c's branch_pool
is a max pool, and `fc` (1008 outputs) / AuxLogits are never evaluated.
"""
import torch

from ..convnet import ConvUnit, conv_bn_shapes

BN_EPS = 1e-3


def _u(name, ci, co, k=1, stride=1, pad=0):
    kh, kw = (k, k) if isinstance(k, int) else k
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    return ConvUnit(name, ci, co, kh, kw, stride, ph, pw)


def _block_a(n, ci, pf):
    return [_u(f"{n}.branch1x1", ci, 64),
            _u(f"{n}.branch5x5_1", ci, 48), _u(f"{n}.branch5x5_2", 48, 64, 5, pad=2),
            _u(f"{n}.branch3x3dbl_1", ci, 64), _u(f"{n}.branch3x3dbl_2", 64, 96, 3, pad=1),
            _u(f"{n}.branch3x3dbl_3", 96, 96, 3, pad=1),
            _u(f"{n}.branch_pool", ci, pf)]


def _block_b(n, ci):
    return [_u(f"{n}.branch3x3", ci, 384, 3, stride=2),
            _u(f"{n}.branch3x3dbl_1", ci, 64), _u(f"{n}.branch3x3dbl_2", 64, 96, 3, pad=1),
            _u(f"{n}.branch3x3dbl_3", 96, 96, 3, stride=2)]


def _block_c(n, ci, c7):
    return [_u(f"{n}.branch1x1", ci, 192),
            _u(f"{n}.branch7x7_1", ci, c7), _u(f"{n}.branch7x7_2", c7, c7, (1, 7), pad=(0, 3)),
            _u(f"{n}.branch7x7_3", c7, 192, (7, 1), pad=(3, 0)),
            _u(f"{n}.branch7x7dbl_1", ci, c7), _u(f"{n}.branch7x7dbl_2", c7, c7, (7, 1), pad=(3, 0)),
            _u(f"{n}.branch7x7dbl_3", c7, c7, (1, 7), pad=(0, 3)), _u(f"{n}.branch7x7dbl_4", c7, c7, (7, 1), pad=(3, 0)),
            _u(f"{n}.branch7x7dbl_5", c7, 192, (1, 7), pad=(0, 3)),
            _u(f"{n}.branch_pool", ci, 192)]


def _block_d(n, ci):
    return [_u(f"{n}.branch3x3_1", ci, 192), _u(f"{n}.branch3x3_2", 192, 320, 3, stride=2),
            _u(f"{n}.branch7x7x3_1", ci, 192), _u(f"{n}.branch7x7x3_2", 192, 192, (1, 7), pad=(0, 3)),
            _u(f"{n}.branch7x7x3_3", 192, 192, (7, 1), pad=(3, 0)), _u(f"{n}.branch7x7x3_4", 192, 192, 3, stride=2)]


def _block_e(n, ci):
    return [_u(f"{n}.branch1x1", ci, 320),
            _u(f"{n}.branch3x3_1", ci, 384), _u(f"{n}.branch3x3_2a", 384, 384, (1, 3), pad=(0, 1)),
            _u(f"{n}.branch3x3_2b", 384, 384, (3, 1), pad=(1, 0)),
            _u(f"{n}.branch3x3dbl_1", ci, 448), _u(f"{n}.branch3x3dbl_2", 448, 384, 3, pad=1),
            _u(f"{n}.branch3x3dbl_3a", 384, 384, (1, 3), pad=(0, 1)), _u(f"{n}.branch3x3dbl_3b", 384, 384, (3, 1), pad=(1, 0)),
            _u(f"{n}.branch_pool", ci, 192)]


def build_units():
    """The 94 conv units in forward order."""
    units = [_u("Conv2d_1a_3x3", 3, 32, 3, stride=2), _u("Conv2d_2a_3x3", 32, 32, 3), _u("Conv2d_2b_3x3", 32, 64, 3, pad=1),
             _u("Conv2d_3b_1x1", 64, 80), _u("Conv2d_4a_3x3", 80, 192, 3)]
    units += _block_a("Mixed_5b", 192, 32) + _block_a("Mixed_5c", 256, 64) + _block_a("Mixed_5d", 288, 64)
    units += _block_b("Mixed_6a", 288)
    units += (_block_c("Mixed_6b", 768, 128) + _block_c("Mixed_6c", 768, 160) + _block_c("Mixed_6d", 768, 160)
              + _block_c("Mixed_6e", 768, 192))
    units += _block_d("Mixed_7a", 768)
    units += _block_e("Mixed_7b", 1280) + _block_e("Mixed_7c", 2048)
    return units


def keys(u):
    """(conv prefix, BatchNorm prefix) of a unit: <name>.conv.weight, <name>.bn.{weight,bias,running_mean,running_var,
    num_batches_tracked}."""
    return f"{u.name}.conv", f"{u.name}.bn"


def state_dict_shapes(units=None, num_batches_tracked=True):
    """{key: shape} of the trunk in pytorch-fid's / torchvision's naming (6 entries per unit with num_batches_tracked)."""
    return conv_bn_shapes(units or build_units(), keys, num_batches_tracked)


def ignored(key):
    """The keys of a pytorch-fid state dict that the trunk does not use (convnet.checked raises on any other stray)."""
    return key.startswith(("fc.", "AuxLogits.")) or key.endswith("num_batches_tracked")


def init_state_dict(seed=0, units=None):
    """Seeded stand-in weights under the upstream names (He-normal convs, unit BatchNorm scale, small random shift and
    running statistics).  Tests calibrate the running statistics themselves; this is only a well-formed checkpoint."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for u in units or build_units():
        sd[f"{u.name}.conv.weight"] = torch.randn(u.co, u.ci, u.kh, u.kw, generator=g) * (2.0 / u.k) ** 0.5
        sd[f"{u.name}.bn.weight"] = torch.ones(u.co)
        sd[f"{u.name}.bn.bias"] = torch.randn(u.co, generator=g) * 0.1
        sd[f"{u.name}.bn.running_mean"] = torch.randn(u.co, generator=g) * 0.1
        sd[f"{u.name}.bn.running_var"] = torch.rand(u.co, generator=g) * 0.5 + 0.75
        sd[f"{u.name}.bn.num_batches_tracked"] = torch.tensor(0)
    return sd
