"""pdmk_image_prep against the reference's torchvision transform written out with PIL + torch on the CPU
(pdm/utils/data_utils.py:68-97: Resize(R, BILINEAR) -> CenterCrop / RandomCrop -> flip -> ToTensor -> Normalize(0.5, 0.5)):
every output element equal, max abs difference 0 in fp32."""
import numpy as np
import pytest
import torch

from PIL import Image

pytestmark = pytest.mark.gpu


def _resized(h, w, R):
    # torchvision's Resize(int) size rule: the short side becomes R, the long side int(R * long / short)
    if w <= h:
        return int(R * h / w), R
    return R, int(R * w / h)


def _reference(img, R, top, left, flip):
    rgb = img.convert("RGB")
    rh, rw = _resized(rgb.height, rgb.width, R)
    r = rgb.resize((rw, rh), Image.BILINEAR) if (rh, rw) != (rgb.height, rgb.width) else rgb
    r = r.crop((left, top, left + R, top + R))
    if flip:
        r = r.transpose(Image.FLIP_LEFT_RIGHT)
    x = torch.from_numpy(np.array(r, np.uint8, copy=True)).permute(2, 0, 1).contiguous().float().div(255)
    return x.sub(0.5).div(0.5)


def _random_image(h, w, seed, mode="RGB"):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    # smooth structure plus noise: interpolation errors show on edges and gradients alike
    yy, xx = np.mgrid[0:h, 0:w]
    a[..., 0] = ((xx * 255) // max(w - 1, 1)).astype(np.uint8)
    img = Image.fromarray(a, "RGB")
    return img if mode == "RGB" else img.convert(mode)


def _run(dev, items, R):
    """items: (PIL image, top, left, flip) -> kernel output [B, 3, R, R] and the packed descriptors."""
    from pdm import _pdmk
    arrays, desc, off = [], [], 0
    for img, top, left, flip in items:
        a = np.ascontiguousarray(np.asarray(img.convert("RGB"), np.uint8))
        h, w = a.shape[:2]
        rh, rw = _resized(h, w, R)
        desc.append([off, h, w, rh, rw, top, left, int(flip)])
        arrays.append(a.reshape(-1))
        off += a.size
        off += (-off) % 4 + 4 * (len(desc) % 2)        # ragged gaps between the images as well
    buf = np.zeros(off + 4, np.uint8)
    for (o, *_), a in zip(desc, arrays):
        buf[o:o + a.size] = a
    desc = torch.tensor(desc, dtype=torch.int64)
    src = torch.from_numpy(buf).to(dev)
    out = torch.full((len(items), 3, R, R), float("nan"), device=dev)
    _pdmk.image_prep(src, desc, desc.to(dev), out)
    torch.cuda.synchronize()
    return out.cpu(), desc


def _check(dev, items, R):
    out, desc = _run(dev, items, R)
    for i, (img, top, left, flip) in enumerate(items):
        ref = _reference(img, R, top, left, flip)
        diff = (out[i] - ref).abs().max().item()
        assert diff == 0.0, (i, tuple(desc[i].tolist()), diff)


def _center(img, R):
    rh, rw = _resized(img.height, img.width, R)
    return int(round((rh - R) / 2.0)), int(round((rw - R) / 2.0))


@pytest.mark.parametrize("h,w,R", [(480, 640, 512), (300, 1000, 512), (53, 37, 64), (64, 64, 64), (97, 97, 48),
                                   (640, 427, 512), (333, 501, 256), (1000, 300, 96), (31, 517, 30)])
def test_center_crop_matches_pil(dev, h, w, R):
    img = _random_image(h, w, seed=h * 7 + w)
    for flip in (0, 1):
        _check(dev, [(img, *_center(img, R), flip)], R)


def test_random_crops_at_both_edges_and_flip(dev):
    R = 128
    items = []
    for s, (h, w) in enumerate([(200, 300), (300, 200), (150, 151)]):
        img = _random_image(h, w, seed=100 + s)
        rh, rw = _resized(h, w, R)
        for top, left in ((0, 0), (rh - R, rw - R), (0, rw - R), (rh - R, 0), ((rh - R) // 3, (rw - R) // 2)):
            for flip in (0, 1):
                items.append((img, top, left, flip))
    _check(dev, items, R)


def test_ragged_batch_of_mixed_sizes_in_one_launch(dev):
    R = 64
    sizes = [(480, 640), (37, 53), (64, 64), (101, 33), (640, 427), (65, 63), (200, 1000), (3, 300)]
    items = []
    for s, (h, w) in enumerate(sizes):
        img = _random_image(h, w, seed=s)
        rh, rw = _resized(h, w, R)
        items.append((img, (s * 7) % (rh - R + 1), (s * 13) % (rw - R + 1), s % 2))
    _check(dev, items, R)


def test_single_image_batch_and_large_downscale(dev):
    # 1000 x 700 -> 104 x 73: ~21 vertical and horizontal taps per output; 2000 x 1600 -> 640 x 512: a band of 4 output rows
    # needs more source rows than the LDS stage holds at R = 512, so the vertical sums run over several chunks
    _check(dev, [(_random_image(1000, 700, seed=5), 3, 0, 1)], 73)
    img = _random_image(2000, 1600, seed=6)
    _check(dev, [(img, *_center(img, 512), 0)], 512)


@pytest.mark.parametrize("mode", ["L", "RGBA", "P", "CMYK"])
def test_non_rgb_inputs_are_converted_on_the_host(dev, mode):
    img = _random_image(90, 120, seed=9, mode=mode)
    _check(dev, [(img, *_center(img, 64), 1)], 64)


def test_invalid_descriptors_are_rejected(dev):
    from pdm import _pdmk
    R = 32
    src = torch.zeros(64 * 48 * 3 + 4, dtype=torch.uint8, device=dev)
    ok = [0, 48, 64, 32, 42, 0, 0, 0]
    out = torch.empty(1, 3, R, R, device=dev)

    def run(d, s=src):
        d = torch.tensor([d], dtype=torch.int64)
        _pdmk.image_prep(s, d, d.to(dev), out)

    run(ok)
    bad = [[0, 48, 64, 32, 42, 1, 0, 0],        # crop below the resized image
           [0, 48, 64, 32, 42, 0, 11, 0],       # crop right of it
           [0, 48, 64, 32, 42, -1, 0, 0],       # negative origin
           [0, 0, 64, 32, 42, 0, 0, 0],         # zero height
           [0, 48, 64, 32, 0, 0, 0, 0],         # zero resized width
           [8, 48, 64, 32, 42, 0, 0, 0],        # image runs past the buffer
           [-4, 48, 64, 32, 42, 0, 0, 0],       # negative offset
           [0, 48, 64, 32, 42, 0, 0, 2]]        # flip is 0 or 1
    for d in bad:
        with pytest.raises(_pdmk.PdmkError):
            run(d)
    with pytest.raises(_pdmk.PdmkError):        # R above the kernel's limit
        _pdmk.image_prep(src, torch.tensor([ok], dtype=torch.int64), torch.tensor([ok], device=dev),
                         torch.empty(1, 3, 2048, 2048, device=dev))
    torch.cuda.synchronize()
