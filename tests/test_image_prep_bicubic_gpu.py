"""pdmk_image_prep_ex with filter 1 against CLIP's transform written out with PIL + numpy on the CPU (Resize(224, BICUBIC)
of the short side -> CenterCrop -> ToTensor -> Normalize(CLIP mean, std) in fp32): every output element equal, max abs
difference 0.  filter 0 through the new entry is pdmk_image_prep bit for bit."""
import numpy as np
import pytest
import torch

from clip_score_fixtures import CLIP_MEAN, CLIP_STD, clip_preprocess, image_array

pytestmark = pytest.mark.gpu


def _pack(arrays, R, crops=None):
    from pdm.utils.data import center_crop_origin, resized_size
    desc, off = [], 0
    for i, a in enumerate(arrays):
        h, w = a.shape[:2]
        rh, rw = resized_size(h, w, R)
        top, left = crops[i] if crops else center_crop_origin(rh, rw, R)
        desc.append([off, h, w, rh, rw, top, left, 0])
        off += a.size
        off += (-off) % 4 + 4 * (len(desc) % 2)        # ragged gaps between the images
    buf = np.zeros(off + 4, np.uint8)
    for (o, *_), a in zip(desc, arrays):
        buf[o:o + a.size] = a.reshape(-1)
    return torch.from_numpy(buf), torch.tensor(desc, dtype=torch.int64)


def _run(dev, arrays, R=224, filt=1, mean=CLIP_MEAN, std=CLIP_STD):
    from pdm import _pdmk
    buf, desc = _pack(arrays, R)
    out = torch.full((len(arrays), 3, R, R), float("nan"), device=dev)
    _pdmk.image_prep_ex(buf.to(dev), desc, desc.to(dev), out, filter=filt, mean=mean, std=std)
    torch.cuda.synchronize()
    return out.cpu()


def _check(dev, sizes, seed=0):
    arrays = [image_array(h, w, seed + i) for i, (h, w) in enumerate(sizes)]
    got = _run(dev, arrays)
    for i, a in enumerate(arrays):
        ref = torch.from_numpy(clip_preprocess(a))
        diff = (got[i] - ref).abs().max().item()
        assert diff == 0, f"image {i} {a.shape}: max abs diff {diff}"


@pytest.mark.parametrize("sizes", [[(512, 512)], [(256, 256)], [(768, 1024)], [(200, 300)], [(150, 100)], [(224, 224)],
                                   [(300, 1)], [(1, 300)], [(1, 1)]])
def test_bicubic_bit_exact(dev, sizes):
    _check(dev, sizes)


def test_bicubic_ragged_batch(dev):
    _check(dev, [(512, 512), (256, 256), (768, 1024), (200, 300), (150, 100), (224, 224), (300, 1), (333, 257)], seed=7)


def test_bicubic_downscale_limit(dev):
    from pdm import _pdmk
    R = 8
    # 63x is the documented bicubic limit (504 / 8); 64x is refused with -1, which bilinear (127x) still takes
    _check_small = [image_array(504, 504, 3)]
    got = _run(dev, _check_small, R=R)
    ref = torch.from_numpy(clip_preprocess(_check_small[0], R))
    assert (got[0] - ref).abs().max().item() == 0
    a = [image_array(512, 512, 4)]
    buf, desc = _pack(a, R)
    out = torch.empty(1, 3, R, R, device=dev)
    with pytest.raises(_pdmk.PdmkError):
        _pdmk.image_prep_ex(buf.to(dev), desc, desc.to(dev), out, filter=1)
    _pdmk.image_prep_ex(buf.to(dev), desc, desc.to(dev), out, filter=0)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def test_bilinear_through_new_entry_is_image_prep(dev):
    from pdm import _pdmk
    arrays = [image_array(h, w, 20 + i) for i, (h, w) in enumerate([(512, 512), (37, 53), (300, 200), (64, 64)])]
    R = 48
    buf, desc = _pack(arrays, R)
    a = torch.full((4, 3, R, R), float("nan"), device=dev)
    b = torch.full((4, 3, R, R), float("nan"), device=dev)
    _pdmk.image_prep(buf.to(dev), desc, desc.to(dev), a)
    _pdmk.image_prep_ex(buf.to(dev), desc, desc.to(dev), b, filter=0, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
