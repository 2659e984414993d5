"""`ResNet50Classifier` (pdm/models/resnet) end to end on the GPU against the unfolded-BatchNorm restatement of
tests/resnet_fixtures.py: logits of the four-bottleneck net and of the full (3, 4, 6, 3) trunk, `classify` against PIL + the
restatement, the prep tensor bit for bit, weights through a file, and the loader's refusals.  Yardstick: 8 x the float32
restatement's own error against float64, floor 8 fp32 ulps; indices exact under the fixtures' gap condition."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_fixtures as fx  # noqa: E402

pytestmark = pytest.mark.gpu
LAYERS = {"tiny": fx.TINY, "full": fx.FULL}


@pytest.fixture(scope="module")
def nets(dev):
    from pdm.models.resnet import ResNet50Classifier
    out = {}
    for name, layers in LAYERS.items():
        sd = fx.calibrated_state_dict(layers)
        m = ResNet50Classifier(device=dev, init=False, layers=layers)
        m.load_state_dict(sd)
        out[name] = (m, sd)
    return out


@pytest.mark.parametrize("size", [(64, 64), (33, 47)], ids=["64x64", "33x47"])
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_logits(dev, nets, name, size):
    model, sd = nets[name]
    x = torch.cat([fx.normalised(fx.image(220 + i, *size)) for i in range(3)])
    ref = fx.oracle_logits(sd, LAYERS[name], x, torch.float64)
    cpu32 = fx.oracle_logits(sd, LAYERS[name], x, torch.float32)
    fx.check_logits(ref, cpu32, f"{name} {size}")
    for B in (1, 3):
        got = model.forward_nhwc(x[:B].permute(0, 2, 3, 1).contiguous().to(dev)).cpu().numpy().astype(np.float64)
        assert got.shape == (B, 1000)
        bad = fx.yardstick(ref[:B], cpu32[:B], got, f"resnet {name} {size} B={B} logits")
        assert not bad, bad
        p64, i64, p32 = fx.check_gaps(ref[:B], cpu32[:B], 5, f"{name} {size} B={B}")
        from pdm import _pdmk
        gp, gi = _pdmk.softmax_topk(torch.from_numpy(got.astype(np.float32)).to(dev), 5)
        assert np.array_equal(gi.cpu().numpy(), i64)
        bad = fx.yardstick(p64, p32, gp.cpu().numpy(), f"resnet {name} {size} B={B} probs")
        assert not bad, bad


@pytest.mark.parametrize("size", [(40, 40), (50, 37)], ids=["40x40", "50x37"])
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_classify(dev, nets, name, size):
    """classify(resize_size=36, crop_size=32) against the preset done with PIL and the restatement; batch_size 2 over three
    images runs a full and a partial batch."""
    model, sd = nets[name]
    imgs = [fx.image(300 + i, *size) for i in range(3)]
    x = torch.cat([fx.preset(im, 36, 32) for im in imgs])
    ref = fx.oracle_logits(sd, LAYERS[name], x, torch.float64)
    cpu32 = fx.oracle_logits(sd, LAYERS[name], x, torch.float32)
    fx.check_logits(ref, cpu32, f"classify {name} {size}")
    p64, i64, p32 = fx.check_gaps(ref, cpu32, 5, f"classify {name} {size}")
    probs, idx = model.classify(imgs, topk=5, resize_size=36, crop_size=32, batch_size=2)
    assert tuple(probs.shape) == (3, 5) and tuple(idx.shape) == (3, 5)
    assert np.array_equal(idx.numpy(), i64), (idx, i64)
    bad = fx.yardstick(p64, p32, probs.numpy(), f"classify {name} {size} probs")
    assert not bad, bad


def test_prep_is_pil_bit_for_bit(dev, nets):
    model, _ = nets["tiny"]
    imgs = [fx.image(200, 40, 40), fx.image(201, 50, 37), fx.image(202, 37, 50), fx.image(203, 36, 36), fx.image(204, 64, 33)]
    got = model.prep(imgs, 36, 32).cpu()
    assert tuple(got.shape) == (5, 32, 32, 3)
    for i, im in enumerate(imgs):
        ref = fx.preset(im, 36, 32)[0].permute(1, 2, 0).contiguous()
        assert torch.equal(got[i].view(torch.int32), ref.view(torch.int32)), f"image {i} {im.shape}"
    with pytest.raises(ValueError, match="smaller than"):
        model.prep(imgs[:1], 30, 32)


def test_classify_reads_files(dev, nets, tmp_path):
    from PIL import Image
    model, _ = nets["tiny"]
    imgs = [fx.image(300 + i, 40, 40) for i in range(2)]
    paths = []
    for i, im in enumerate(imgs):
        paths.append(str(tmp_path / f"{i}_0.png"))
        Image.fromarray(im).save(paths[-1])
    pa, ia = model.classify(imgs, topk=3, resize_size=36, crop_size=32)
    pf, jf = model.classify(paths, topk=3, resize_size=36, crop_size=32)
    assert torch.equal(pa, pf) and torch.equal(ia, jf)


def test_weights_round_trip_through_file(dev, nets, tmp_path):
    from pdm.models.resnet import ResNet50Classifier
    model, sd = nets["full"]
    path = str(tmp_path / "resnet50.pth")
    torch.save(sd, path)
    loaded = ResNet50Classifier.from_pretrained(path, device=dev)
    assert torch.equal(loaded.arena, model.arena)
    x = fx.normalised(fx.image(50, 64, 64)).permute(0, 2, 3, 1).contiguous().to(dev)
    assert torch.equal(loaded.forward_nhwc(x), model.forward_nhwc(x))


def test_state_dict_is_checked(dev, nets):
    from pdm.models.resnet import ResNet50Classifier
    _, sd = nets["tiny"]
    m = ResNet50Classifier(device=dev, init=False, layers=fx.TINY)
    missing = dict(sd)
    del missing["layer2.0.downsample.0.weight"]
    with pytest.raises(KeyError, match="layer2.0.downsample.0.weight"):
        m.load_state_dict(missing)
    wrong = dict(sd)
    wrong["layer3.0.conv2.weight"] = torch.zeros(256, 256, 1, 1)
    with pytest.raises(ValueError, match="layer3.0.conv2.weight"):
        m.load_state_dict(wrong)
    wrong = dict(sd)
    wrong["fc.weight"] = torch.zeros(1008, 2048)
    with pytest.raises(ValueError, match="fc.weight"):
        m.load_state_dict(wrong)
    stray = dict(sd, **{"layer9.0.conv1.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="layer9"):
        m.load_state_dict(stray)
    no_counter = {n: t for n, t in sd.items() if not n.endswith("num_batches_tracked")}
    m.load_state_dict(no_counter)                            # num_batches_tracked is optional


def test_from_pretrained_never_fetches(dev, tmp_path, monkeypatch):
    """A missing file is FileNotFoundError naming the file and the flag; no socket is opened on the way."""
    from pdm.models.resnet import ResNet50Classifier

    def no_socket(*a, **kw):
        raise AssertionError("from_pretrained opened a socket")

    monkeypatch.setattr(socket, "socket", no_socket)
    monkeypatch.setattr(socket, "create_connection", no_socket)
    with pytest.raises(FileNotFoundError, match=r"resnet50-11ad3fa6\.pth.*--resnet_weights"):
        ResNet50Classifier.from_pretrained(str(tmp_path / "absent.pth"), device=dev)
    monkeypatch.setenv("HOME", str(tmp_path))
    with pytest.raises(FileNotFoundError, match=r"resnet50-11ad3fa6\.pth"):
        ResNet50Classifier.from_pretrained(device=dev)
