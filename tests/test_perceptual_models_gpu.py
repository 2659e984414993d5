"""`VGG19Style` and `AlexNetLPIPS` (pdm/models/perceptual) end to end on the GPU: uint8 images -> prep -> trunk -> metric heads,
against the numbers of the reference's own styleloss.py (tests/golden/perceptual_ref.npz) and against the float64 restatements
of tests/perceptual_fixtures.py, with the project's yardstick (8 x the float32 restatement's own error, floor 8 fp32 ulps)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perceptual_fixtures as fx  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perceptual_ref.npz")


@pytest.fixture(scope="module")
def vgg(dev):
    from pdm.models.perceptual import VGG19Style
    sd = fx.vgg_state_dict()
    model = VGG19Style(device=dev, init=False)
    model.load_state_dict(sd)
    return model, sd


@pytest.fixture(scope="module")
def alex(dev):
    from pdm.models.perceptual import AlexNetLPIPS
    sd, lin = fx.alexnet_state_dict(), fx.lin_state_dict()
    model = AlexNetLPIPS(device=dev, init=False)
    model.load_state_dict(sd, lin)
    return model, sd, lin


def _vgg_run(model, a, b, size):
    return np.stack([t.cpu().numpy() for t in model.forward_nhwc(model.prep(a, b, size))], axis=1)       # [B, 3]


def _assert_ok(bad):
    assert not bad, bad


def test_vgg_against_the_reference_code(dev, vgg):
    """The three golden pairs: the reference's own functions in float64 are the oracle, the same in float32 the yardstick."""
    model, _ = vgg
    z = np.load(GOLDEN)
    a, b = fx.golden_pairs()
    for B in (1, 3):
        got = _vgg_run(model, a[:B], b[:B], 48)
        assert got.shape == (B, 3)
        for j, name in enumerate(("style", "content", "total")):
            _assert_ok(fx.yardstick(z["ref64"][:B, j], z["ref32"][:B, j], got[:, j], f"vgg golden B={B} {name}"))


@pytest.mark.parametrize("size", [48, 37])
def test_vgg_against_the_restatement(dev, vgg, size):
    """48: even maps all the way; 37: both pools drop a row and a column (37 -> 18 -> 9).  Batches of 1 and 3."""
    model, sd = vgg
    a, b = fx.pairs(20 + size, 3, size)
    ref, cpu32 = (fx.vgg_losses(sd, a, b, size, d) for d in (torch.float64, torch.float32))
    for B in (1, 3):
        got = _vgg_run(model, a[:B], b[:B], size)
        for j, name in enumerate(("style", "content", "total")):
            _assert_ok(fx.yardstick(ref[:B, j], cpu32[:B, j], got[:, j], f"vgg {size}px B={B} {name}"))
    same = _vgg_run(model, a, [x.copy() for x in a], size)
    assert np.array_equal(same, np.zeros((3, 3))), "identical images must give exactly 0.0"


def test_lpips_against_the_restatement(dev, alex):
    model, sd, lin = alex
    a, b = fx.pairs(31, 3, 64)
    ref, cpu32 = (fx.lpips(sd, lin, a, b, 64, d) for d in (torch.float64, torch.float32))
    for B in (1, 3):
        got = model.forward_nhwc(model.prep(a[:B], b[:B], 64)).cpu().numpy()
        assert got.shape == (B,)
        _assert_ok(fx.yardstick(ref[:B], cpu32[:B], got, f"lpips 64px B={B}"))
    same = model.forward_nhwc(model.prep(a, [x.copy() for x in a], 64)).cpu().numpy()
    assert np.array_equal(same, np.zeros(3))


def _border_image(size, rgb, seed):
    """Constant at the uint8 level nearest to the normalisation mean, except the outermost row / column ring (noise): the
    normalised interior is ~0, so what the first conv sees at the border is the zero padding against the ring.  A mean folded
    into the first conv's bias instead of subtracted before the padding is wrong exactly there."""
    img = np.empty((size, size, 3), np.uint8)
    img[:] = np.asarray(rgb, np.uint8)
    ring = fx.noise_image(seed, size)
    for s in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        img[s] = ring[s]
    return img


def test_border_pixels_see_zero_padding_of_the_normalised_image(dev, vgg, alex):
    model, sd = vgg
    rgb = [round(m * 255) for m in fx.IMAGENET_MEAN]
    a, b = [_border_image(48, rgb, 1)], [fx.noise_image(2, 48)]
    ref, cpu32 = (fx.vgg_losses(sd, a, b, 48, d) for d in (torch.float64, torch.float32))
    got = _vgg_run(model, a, b, 48)
    for j, name in enumerate(("style", "content", "total")):
        _assert_ok(fx.yardstick(ref[:, j], cpu32[:, j], got[:, j], f"vgg border {name}"))
    model, sd, lin = alex
    rgb = [round((0.5 + 0.5 * s) * 255) for s in fx.SHIFT]
    a, b = [_border_image(64, rgb, 3)], [fx.noise_image(4, 64)]
    ref, cpu32 = (fx.lpips(sd, lin, a, b, 64, d) for d in (torch.float64, torch.float32))
    _assert_ok(fx.yardstick(ref, cpu32, model.forward_nhwc(model.prep(a, b, 64)).cpu().numpy(), "lpips border"))


def test_weights_round_trip_through_files(dev, vgg, alex, tmp_path):
    from pdm.models.perceptual import AlexNetLPIPS, VGG19Style
    model, sd = vgg
    a, b = fx.pairs(40, 2, 48)
    torch.save(sd, tmp_path / "vgg19.pth")
    loaded = VGG19Style.from_pretrained(str(tmp_path / "vgg19.pth"), device=dev)
    assert torch.equal(loaded.arena, model.arena)
    assert np.array_equal(_vgg_run(loaded, a, b, 48), _vgg_run(model, a, b, 48))
    for key in ("features.10.weight", "features.0.bias"):
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            VGG19Style(device=dev, init=False).load_state_dict({n: t for n, t in sd.items() if n != key})
    with pytest.raises(ValueError, match="features.5.weight"):
        VGG19Style(device=dev, init=False).load_state_dict(dict(sd, **{"features.5.weight": torch.zeros(128, 64, 3, 1)}))
    with pytest.raises(FileNotFoundError, match="vgg19-dcbb9e9d.pth"):
        VGG19Style.from_pretrained(str(tmp_path / "absent.pth"), device=dev)

    model, sd, lin = alex
    torch.save(sd, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    loaded = AlexNetLPIPS.from_pretrained(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"), device=dev)
    assert torch.equal(loaded.arena, model.arena)
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        AlexNetLPIPS(device=dev, init=False).load_state_dict(sd, {n: t for n, t in lin.items() if not n.startswith("lin3")})
    with pytest.raises(KeyError, match=r"features\.6\.weight"):
        AlexNetLPIPS(device=dev, init=False).load_state_dict({n: t for n, t in sd.items() if n != "features.6.weight"}, lin)
    with pytest.raises(FileNotFoundError, match="alex.pth"):
        AlexNetLPIPS.from_pretrained(str(tmp_path / "alexnet.pth"), str(tmp_path / "absent.pth"), device=dev)
