"""Fixtures of the perceptual-metric tests: plain-torch CPU restatements of the two metrics, seeded weights under the upstream
key names, and seeded images.  Independent of pdm/models/perceptual (its tables are not imported).

* `vgg_losses`: the reference's styleloss.py in closed form: ImageNet Normalize of the [0, 1] image, torchvision VGG-19
  features 0 .. 10, Gram matrices of the PRE-ReLU conv outputs (per image, divided by C * H * W), style = sum over the five
  convs of mse(G_edited, G_original), content = mse at conv_4, total = 1e6 style + content.  tests/golden/perceptual_ref.npz
  holds the numbers the reference's own code gives for `golden_pairs()`; test_perceptual_host.py ties the two together.
* `lpips`: lpips v0.1 with net='alex', restated from the package's formula (the package is not available to pin it):
  ScalingLayer of the [-1, 1] image, AlexNet features with taps behind each ReLU, normalize_tensor (x / (||x||_2 + 1e-10) over
  the channels), the squared difference through the 1 x 1 `lin` convs, spatial mean, summed over the five layers.
Each runs in float64 (the oracle) and float32 (the yardstick: its distance from float64 sizes the tolerances).
Weights: He-normal convs, small biases, uniform lin weights.  Images: uniform uint8 noise; a pair is two independent images or
an image and a copy perturbed by up to +-25 levels - never near-identical (there G_0 - G_1 cancels and float32 is no yardstick).
"""
import numpy as np
import torch
import torch.nn.functional as F

ALEX = [("features.0", 3, 64, 11, 4, 2), ("features.3", 64, 192, 5, 1, 2), ("features.6", 192, 384, 3, 1, 1),
        ("features.8", 384, 256, 3, 1, 1), ("features.10", 256, 256, 3, 1, 1)]
VGG = [("features.0", 3, 64), ("features.2", 64, 64), ("features.5", 64, 128), ("features.7", 128, 128), ("features.10", 128, 256),
       ("features.12", 256, 256)]           # features.12 lies behind conv_5: the reference trims it, the loader ignores it
IMAGENET_MEAN, IMAGENET_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SHIFT, SCALE = [-0.030, -0.088, -0.188], [0.458, 0.448, 0.450]


def _convs(table, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, ci, co, *rest in table:
        k = rest[0] if rest else 3
        sd[name + ".weight"] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[name + ".bias"] = torch.randn(co, generator=g) * 0.1
    return sd


def alexnet_state_dict(seed=11):
    sd = _convs(ALEX, seed)
    sd["classifier.1.weight"] = torch.zeros(4, 4)          # torchvision's file has the classifier too: ignored
    return sd


def lin_state_dict(seed=12):
    g = torch.Generator().manual_seed(seed)
    return {f"lin{i}.model.1.weight": torch.rand(1, t[2], 1, 1, generator=g) for i, t in enumerate(ALEX)}


def vgg_state_dict(seed=13):
    return _convs(VGG, seed)


def noise_image(seed, size):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (size, size, 3), generator=g, dtype=torch.uint8).numpy()


def perturbed(img, seed, amount=25):
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(-amount, amount + 1, img.shape, generator=g).numpy()
    return np.clip(img.astype(np.int64) + d, 0, 255).astype(np.uint8)


def pairs(seed, n, size):
    """n pairs (original, edited): even ones independent, odd ones perturbed by +-25 levels."""
    a = [noise_image(seed * 1000 + 2 * i, size) for i in range(n)]
    b = [perturbed(a[i], seed * 1000 + 2 * i + 1) if i % 2 else noise_image(seed * 1000 + 2 * i + 1, size) for i in range(n)]
    return a, b


def golden_pairs():
    """The three 48 x 48 pairs of tests/golden/perceptual_ref.npz."""
    return pairs(5, 3, 48)


def to_tensor(img_u8, size, dtype):
    """Resize(size) (Pillow bilinear) + ToTensor: float32 in [0, 1] whatever `dtype` is (that IS the loader), then cast."""
    from PIL import Image
    im = Image.fromarray(img_u8)
    if im.size != (size, size):
        im = im.resize((size, size), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(im, np.uint8).copy()).permute(2, 0, 1)[None].to(torch.float32).div(255)
    return x.to(dtype)


def _gram(x):
    b, c, h, w = x.shape
    f = x.reshape(b, c, h * w)
    return torch.bmm(f, f.transpose(1, 2)) / (c * h * w)


@torch.no_grad()
def vgg_losses(sd, originals, edited, size, dtype):
    """float64 numpy [N, 3]: style, content, total of every pair, evaluated in `dtype`."""
    out = []
    mean, std = (torch.tensor(v, dtype=dtype).reshape(1, 3, 1, 1) for v in (IMAGENET_MEAN, IMAGENET_STD))
    for a, b in zip(originals, edited):
        x = torch.cat([to_tensor(a, size, dtype), to_tensor(b, size, dtype)])
        x = (x - mean) / std
        style = torch.zeros((), dtype=dtype)
        content = None
        for i, (name, *_) in enumerate(VGG[:5]):
            if i:
                x = F.relu(x)
            if i in (2, 4):
                x = F.max_pool2d(x, 2, 2)
            x = F.conv2d(x, sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype), 1, 1)
            g = _gram(x)
            style = style + F.mse_loss(g[1], g[0])
            if i == 3:
                content = F.mse_loss(x[1], x[0])
        total = style * 1000000 + content * 1
        out.append([style.double().item(), content.double().item(), total.double().item()])
    return np.asarray(out, np.float64)


@torch.no_grad()
def alex_taps(sd, x):
    taps = []
    for i, (name, ci, co, k, s, p) in enumerate(ALEX):
        if i in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype), s, p))
        taps.append(x)
    return taps


@torch.no_grad()
def lpips(sd, lin, images_a, images_b, size, dtype):
    """float64 numpy [N]: lpips.LPIPS(net='alex')(a, b) with the inputs scaled to [-1, 1], evaluated in `dtype`."""
    shift, scale = (torch.tensor(v, dtype=dtype).reshape(1, 3, 1, 1) for v in (SHIFT, SCALE))
    out = []
    for a, b in zip(images_a, images_b):
        x = torch.cat([to_tensor(a, size, dtype), to_tensor(b, size, dtype)])
        x = ((x - 0.5) * 2 - shift) / scale
        val = torch.zeros((), dtype=dtype)
        for i, t in enumerate(alex_taps(sd, x)):
            n = t / (torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True)) + 1e-10)
            d = (n[0:1] - n[1:2]) ** 2
            val = val + F.conv2d(d, lin[f"lin{i}.model.1.weight"].to(dtype)).mean((2, 3)).reshape(())
        out.append(val.double().item())
    return np.asarray(out, np.float64)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def yardstick(ref64, cpu32, got, what):
    """The project's yardstick, as tests/test_fid_gpu.py forms it, for ONE quantity over a batch (never mix quantities of
    different scales in one call): scale = max |ref64|; the largest |got - ref64| of the batch may be at most 8 x the largest
    |cpu32 - ref64|, floor 8 fp32 ulps of the scale.  The fixture condition - every float32 value within 1e-5 relative of its
    float64 value - is asserted first.  Prints every figure; returns the list of failures (empty: passed)."""
    r, c, g = (np.asarray(np.ravel(v), np.float64) for v in (ref64, cpu32, got))
    assert r.shape == c.shape == g.shape and r.size, (r.shape, c.shape, g.shape)
    for i in range(r.size):
        assert abs(c[i] - r[i]) <= 1e-5 * abs(r[i]), f"fixture: {what}[{i}] float32 {c[i]!r} is not within 1e-5 of float64 {r[i]!r}"
        print(f"{what}[{i}]: ref {r[i]:.9e} got {g[i]:.9e} rel err {abs(g[i] - r[i]) / abs(r[i]):.3e} "
              f"(cpu fp32 {abs(c[i] - r[i]) / abs(r[i]):.3e})")
    scale = np.abs(r).max()
    yard = max(8 * np.abs(c - r).max(), 8 * ulp32(scale))
    err = np.abs(g - r).max()
    print(f"{what}: err/max {err / scale:.3e}, yardstick/max {yard / scale:.3e}")
    return [] if err <= yard else [(what, err, yard)]
