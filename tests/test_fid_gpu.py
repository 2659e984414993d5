"""FID on the GPU: the new kernels one by one against torch on the CPU (float64 oracle; torch's own float32 round-off is the
yardstick), the whole Inception against the restatement of tests/fid_fixtures.py, and make_custom_stats.py + fid.py end to
end on temporary directories."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_fixtures as fx  # noqa: E402

pytestmark = pytest.mark.gpu
SCRIPTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unlearn-ft_amd", "scripts", "metrics")


def _k():
    from pdm import _pdmk
    return _pdmk


def _ulp(x):
    return float(np.spacing(np.float32(x)))


# ---------------------------------------------------------------------------------------------------- resize
def test_resize_bilinear_u8(dev):
    """Ragged batch in one launch against F.interpolate(float32, bilinear, align_corners=False) on the CPU -> clip -> / 255
    -> 2x - 1.  Bound 2.5e-6 on the [-1, 1] scale: 16 fp32 ulp of 255 scaled by 2 / 255, plus 4 ulp of 1."""
    from pdm.utils.fid_utils import pack_images, prep_images
    g = torch.Generator().manual_seed(5)
    sizes = [(512, 512), (427, 640), (768, 1024), (299, 299), (64, 64), (1, 1), (1, 37), (41, 1), (1000, 3)]
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy() for h, w in sizes]
    packed, desc = pack_images(imgs)
    got = prep_images(packed, desc, dev).cpu()
    assert got.shape == (len(sizes), 299, 299, 3)
    worst = 0.0
    for i, im in enumerate(imgs):
        x = torch.from_numpy(im).permute(2, 0, 1)[None].float()
        ref = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False).clamp(0, 255) / 255 * 2 - 1
        err = (got[i].permute(2, 0, 1)[None] - ref).abs().max().item()
        print(f"resize {sizes[i]}: max abs err {err:.3e}")
        worst = max(worst, err)
    assert worst <= 2.5e-6, worst


def test_resize_bilinear_u8_bad_arguments(dev):
    k = _k()
    from pdm.utils.fid_utils import pack_images
    packed, desc = pack_images([np.zeros((4, 4, 3), np.uint8)])
    buf = packed.to(dev)
    out = torch.empty(1, 299, 299, 3, device=dev)
    bad = desc.clone()
    bad[0, 1] = 1 << 12                    # taller than the buffer holds
    with pytest.raises(k.PdmkError):
        k.resize_bilinear_u8(buf[64:], bad, bad.to(dev), out)


# ---------------------------------------------------------------------------------------------------- conv
# (Ci, Co, kh, kw, stride, ph, pw, H, W): every geometry of the network with its real channel counts
CONV_CASES = {
    "1a_3x3_s2_ci3": (3, 32, 3, 3, 2, 0, 0, 75, 75),
    "2a_3x3": (32, 32, 3, 3, 1, 0, 0, 37, 37),
    "2b_3x3_p1": (32, 64, 3, 3, 1, 1, 1, 37, 37),
    "3b_1x1_co80": (64, 80, 1, 1, 1, 0, 0, 35, 35),
    "4a_3x3_ci80": (80, 192, 3, 3, 1, 0, 0, 35, 35),
    "5b_5x5_p2": (48, 64, 5, 5, 1, 2, 2, 35, 35),
    "6a_3x3_s2": (288, 384, 3, 3, 2, 0, 0, 35, 35),
    "6b_1x7": (128, 128, 1, 7, 1, 0, 3, 17, 17),
    "6c_7x1": (160, 192, 7, 1, 1, 3, 0, 17, 17),
    "6e_1x1_289px": (768, 192, 1, 1, 1, 0, 0, 17, 17),
    "7a_3x3_s2": (192, 320, 3, 3, 2, 0, 0, 17, 17),
    "7b_1x3": (384, 384, 1, 3, 1, 0, 1, 8, 8),
    "7b_3x1": (384, 384, 3, 1, 1, 1, 0, 8, 8),
    "7b_3x3_p1_ci448": (448, 384, 3, 3, 1, 1, 1, 8, 8),
    "7c_1x1_ci2048": (2048, 320, 1, 1, 1, 0, 0, 8, 8),
}


def _conv_case(dev, case, B, in_off, in_extra, seed=0):
    k = _k()
    Ci, Co, kh, kw, s, ph, pw, H, W = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Ci, generator=g).abs()
    w = torch.randn(Co, Ci, kh, kw, generator=g) * (2.0 / (Ci * kh * kw)) ** 0.5
    b = torch.randn(Co, generator=g) * 0.2
    xn = x.permute(0, 3, 1, 2)
    ref = F.relu(F.conv2d(xn.double(), w.double(), b.double(), s, (ph, pw)))
    cpu32 = F.relu(F.conv2d(xn, w, b, s, (ph, pw))).double()
    Ho, Wo = ref.shape[2:]
    scale = ref.abs().max().item()
    yard = max(8 * (cpu32 - ref).abs().max().item(), 8 * _ulp(scale))
    # input: a column slice [in_off, in_off + Ci) of a buffer with rows of lda; output: columns [16, 16 + Co) of rows of ldc
    lda = Ci + in_extra
    xb = torch.full((B * H * W, lda), 7.0)
    xb[:, in_off:in_off + Ci] = x.reshape(-1, Ci)
    xb = xb.to(dev)
    ldc, o0, canary = Co + 40, 16, -123.25
    yb = torch.full((B * Ho * Wo, ldc), canary, device=dev)
    wk = w.permute(0, 2, 3, 1).reshape(Co, -1).contiguous().to(dev)
    k.conv2d_fwd(xb[:, in_off:in_off + Ci], lda, wk, b.to(dev), yb[:, o0:o0 + Co], ldc, B, H, W, Ci, Co, kh, kw, s, ph, pw, relu=True)
    yb = yb.cpu()
    got = yb[:, o0:o0 + Co].reshape(B, Ho, Wo, Co).permute(0, 3, 1, 2).double()
    err = (got - ref).abs().max().item()
    outside = torch.cat([yb[:, :o0], yb[:, o0 + Co:]], 1)
    return err, yard, scale, bool((outside == canary).all())


@pytest.mark.parametrize("name", sorted(CONV_CASES))
@pytest.mark.parametrize("B,in_off,in_extra", [(1, 0, 0), (3, 8, 24)], ids=["b1_dense", "b3_sliced"])
def test_conv2d_fwd(dev, name, B, in_off, in_extra):
    """Error against F.conv2d float64, relative to the output's max abs: at most 8 x that of F.conv2d float32 (floor: 8 fp32
    ulp of the output's max abs); B = 3 leaves an M tail in every case; columns outside the output slice keep the canary."""
    err, yard, scale, clean = _conv_case(dev, CONV_CASES[name], B, in_off, in_extra)
    print(f"conv {name} B={B}: err/max {err / scale:.3e}, yardstick/max {yard / scale:.3e}")
    assert clean, "columns outside the output slice were written"
    assert err <= yard, (err, yard)


# maps large enough for the 128-row tiles (the cases above all take the 64-row ones: fewer than 512 workgroups otherwise)
LARGE_CASES = {
    "1a_299px_ci3": ((3, 32, 3, 3, 2, 0, 0, 299, 299), 4),
    "2b_147px": ((32, 64, 3, 3, 1, 1, 1, 147, 147), 4),
    "4a_73px_ci80": ((80, 192, 3, 3, 1, 0, 0, 73, 73), 5),
    "3b_1x1_co80_73px": ((64, 80, 1, 1, 1, 0, 0, 73, 73), 13),
}


@pytest.mark.parametrize("name", sorted(LARGE_CASES))
def test_conv2d_fwd_large_maps(dev, name):
    case, B = LARGE_CASES[name]
    Ci, Co, kh, kw, s, ph, pw, H, W = case
    M = B * ((H + 2 * ph - kh) // s + 1) * ((W + 2 * pw - kw) // s + 1)
    assert -(-M // 128) * -(-Co // 64) >= 512 and M % 128, "fixture: not a 128-row-tile case with an M tail"
    err, yard, scale, clean = _conv_case(dev, case, B, 8, 24, seed=2)
    print(f"conv large {name} B={B}: err/max {err / scale:.3e}, yardstick/max {yard / scale:.3e}")
    assert clean and err <= yard, (err, yard, clean)


def test_conv2d_fwd_unaligned_slice(dev):
    """An input slice that is not 16-byte aligned (offset 3, odd row stride) takes the element-gather path."""
    err, yard, scale, clean = _conv_case(dev, CONV_CASES["5b_5x5_p2"], 2, 3, 5, seed=1)
    print(f"conv unaligned: err/max {err / scale:.3e}, yardstick/max {yard / scale:.3e}")
    assert clean and err <= yard, (err, yard, clean)


def test_conv2d_fwd_bad_arguments(dev):
    k = _k()
    x = torch.zeros(64, 8, device=dev)
    w = torch.zeros(8, 8, device=dev)
    y = torch.zeros(64, 8, device=dev)
    with pytest.raises(k.PdmkError):
        k.conv2d_fwd(x, 4, w, None, y, 8, 1, 8, 8, 8, 8, 1, 1, 1, 0, 0)          # lda < Ci
    with pytest.raises(k.PdmkError):
        k.conv2d_fwd(x, 8, w, None, y, 8, 2, 8, 8, 8, 8, 1, 1, 1, 0, 0)          # B larger than the buffers


# ---------------------------------------------------------------------------------------------------- pools
@pytest.mark.parametrize("B,H,C,stride,pad", [(2, 35, 192, 2, 0), (3, 17, 768, 2, 0), (2, 8, 2048, 1, 1), (1, 147, 64, 2, 0)])
def test_pool2d_max_bit_equal(dev, B, H, C, stride, pad):
    k = _k()
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, H, H, C, generator=g)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, stride, pad).permute(0, 2, 3, 1).contiguous()
    Ho = ref.shape[1]
    ldx, ldy = C + 8, C + 12                                 # strided in and out
    xb = torch.zeros(B * H * H, ldx)
    xb[:, 4:4 + C] = x.reshape(-1, C)
    xb = xb.to(dev)
    yb = torch.full((B * Ho * Ho, ldy), -5.0, device=dev)
    k.pool2d(xb[:, 4:4 + C], ldx, yb[:, 8:8 + C], ldy, B, H, H, C, "max", stride, pad)
    yb = yb.cpu()
    assert torch.equal(yb[:, 8:8 + C].reshape(ref.shape), ref)
    assert bool((yb[:, :8] == -5.0).all()) and bool((yb[:, 8 + C:] == -5.0).all())


@pytest.mark.parametrize("B,H,C", [(2, 35, 256), (3, 17, 768), (2, 8, 1280)])
def test_pool2d_avg_valid_count(dev, B, H, C):
    """Non-negative inputs (as after ReLU): <= 4 fp32 ulp of the window's maximum against torch count_include_pad=False."""
    k = _k()
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, H, H, C, generator=g).abs()
    xn = x.permute(0, 3, 1, 2)
    ref = F.avg_pool2d(xn.double(), 3, 1, 1, count_include_pad=False)
    wmax = F.max_pool2d(xn, 3, 1, 1)
    y = torch.empty(B * H * H, C, device=dev)
    k.pool2d(x.reshape(-1, C).to(dev), C, y, C, B, H, H, C, "avg", 1, 1)
    got = y.cpu().reshape(B, H, H, C).permute(0, 3, 1, 2).double()
    tol = torch.from_numpy(np.spacing(wmax.numpy()).astype(np.float64)) * 4
    worst = ((got - ref).abs() / tol).max().item()
    print(f"avg pool {H}x{H}x{C}: worst error {worst * 4:.2f} ulp of the window max")
    assert worst <= 1.0
    ones = torch.ones(B * H * H, C, device=dev)
    k.pool2d(ones, C, y, C, B, H, H, C, "avg", 1, 1)
    assert torch.equal(y.cpu(), torch.ones(B * H * H, C)), "border divisor is not the valid-tap count"


def test_global_avgpool(dev):
    k = _k()
    g = torch.Generator().manual_seed(3)
    B, HW, C = 5, 64, 2048
    x = torch.randn(B, HW, C, generator=g).abs()
    ref = x.double().mean(1)
    cpu32 = x.mean(1).double()
    scale = ref.abs().max().item()
    yard = max(8 * (cpu32 - ref).abs().max().item(), 8 * _ulp(scale))
    y = torch.empty(B, C, device=dev)
    k.global_avgpool(x.reshape(-1, C).to(dev), C, y, B, HW, C)
    err = (y.cpu().double() - ref).abs().max().item()
    print(f"global avgpool: err/max {err / scale:.3e}, yardstick/max {yard / scale:.3e}")
    assert err <= yard, (err, yard)


# ---------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("D,N", [(2048, 300), (100, 70)])
def test_fid_accumulate(dev, D, N):
    """mu / sigma from the device's fp64 sums against np.mean / np.cov of the same fp32 features: <= 1e-11 relative to
    max|sigma| (fp64, one-pass form: eps * N * mean^2 / var); a second run gives the same bits."""
    k = _k()
    from pdm.utils.fid_utils import finish_statistics
    g = torch.Generator().manual_seed(D)
    f = (torch.randn(N, D, generator=g) * 0.2 + torch.rand(1, D, generator=g) * 0.8 + 0.1).clamp_min(0)
    fd = f.to(dev)

    def run():
        total = torch.zeros(D, device=dev, dtype=torch.float64)
        outer = torch.zeros(D, D, device=dev, dtype=torch.float64)
        for i in range(0, N, 64):
            k.fid_accumulate(fd[i:i + 64], total, outer)
        return total.cpu(), outer.cpu()

    t1, o1 = run()
    t2, o2 = run()
    assert torch.equal(t1, t2) and torch.equal(o1, o2)
    mu, sigma = finish_statistics(t1, o1, N)
    f64 = f.double().numpy()
    rmu, rs = f64.mean(axis=0), np.cov(f64, rowvar=False)
    emu = np.abs(mu - rmu).max() / np.abs(rmu).max()
    es = np.abs(sigma - rs).max() / np.abs(rs).max()
    print(f"fid_accumulate D={D} N={N}: mu {emu:.3e}, sigma {es:.3e}")
    assert emu <= 1e-11 and es <= 1e-11, (emu, es)


# ---------------------------------------------------------------------------------------------------- network
@pytest.fixture(scope="module")
def net(dev):
    from pdm.models.inception.inception_v3 import InceptionV3FID
    sd = fx.calibrated_state_dict()
    model = InceptionV3FID(device=dev, init=False)
    model.load_state_dict(sd)
    return model, sd


def test_inception_features(dev, net):
    """Seeded weights with calibrated BatchNorm statistics, 16 structured images of mixed sizes, B = 1, 5, 16: max abs error
    against the float64 restatement relative to max|feature| <= 8 x the float32 restatement's own."""
    model, sd = net
    imgs = fx.images(3, 16)
    ref = fx.oracle_features(sd, imgs, torch.float64)
    cpu32 = fx.oracle_features(sd, imgs, torch.float32)
    assert (ref.std(axis=0) >= 0.1 * ref.mean(axis=0)).all(), "fixture: a feature dimension does not depend on the image"
    scale = np.abs(ref).max()
    yard = 8 * np.abs(cpu32 - ref).max() / scale
    for B in (1, 5, 16):
        got = model.features(imgs[:B]).cpu().double().numpy()
        assert got.shape == (B, 2048)
        err = np.abs(got - ref[:B]).max() / scale
        print(f"inception B={B}: err/max {err:.3e}, yardstick (8 x cpu fp32) {yard:.3e}")
        assert err <= yard, (B, err, yard)


# ---------------------------------------------------------------------------------------------------- Pillow resize
@pytest.mark.parametrize("src,size", [((427, 640), (512, 512)), ((375, 500), (256, 384)), ((80, 100), (300, 200)),
                                      ((120, 90), (90, 120))], ids=["coco_to_512", "to_256x384", "upscale", "identity"])
def test_image_resize_u8_matches_pillow(dev, src, size):
    """pdmk_image_resize_u8 against PIL.Image.resize(size) (default filter, bicubic): every byte equal.  src = (H, W), size = (W, H)."""
    from PIL import Image
    sys.path.insert(0, SCRIPTS)
    import resize_and_save_images as rs
    from pdm.utils.fid_utils import pack_images
    imgs = [fx.structured_image(11 + i, *src) for i in range(3)]
    packed, desc = pack_images(imgs)
    got = rs.resize_batch(packed, desc, size, dev).cpu().numpy()
    for i, im in enumerate(imgs):
        ref = np.array(Image.fromarray(im).resize(size))
        assert got[i].shape == ref.shape
        assert np.abs(got[i].astype(int) - ref.astype(int)).max() == 0


# ---------------------------------------------------------------------------------------------------- end to end
def test_scripts_end_to_end(dev, net, tmp_path):
    """48 "real" and 48 "generated" .npy images (two seeded families, mixed sizes) through make_custom_stats.py and fid.py
    with the weights read from a file: mu / sigma against the float64 oracle pipeline within 8 x the CPU float32 pipeline's
    own error, FID within 2e-5 relative of the oracle's features pushed through the same frechet_distance (N = 48 < 2048:
    scipy's sqrtm is itself unstable there), the fid.txt line, and an identical value on a second run."""
    sys.path.insert(0, SCRIPTS)
    import fid as fid_script
    import make_custom_stats as stats_script
    from pdm.utils.fid_utils import frechet_distance, load_stats, stats_path
    _, sd = net
    real, gen = fx.images(21, 48, family=0), fx.images(22, 48, family=1)
    rdir, gdir, sdir, out = (tmp_path / n for n in ("real", "gen", "stats", "results"))
    for d, imgs in ((rdir, real), (gdir, gen)):
        d.mkdir()
        for i, im in enumerate(imgs):
            np.save(d / f"{i:05d}.npy", im)
    wfile = tmp_path / "pt_inception.pth"
    torch.save(sd, wfile)
    extra = ["--stats_dir", str(sdir), "--inception_weights", str(wfile), "--batch_size", "20", "--num_workers", "2"]
    npz = stats_script.main(["--name", "Toy-48", "--data_dir", str(rdir)] + extra)
    assert npz == stats_path("Toy-48", "legacy_pytorch", str(sdir)) and npz.endswith("toy-48_legacy_pytorch_custom_na.npz")
    mu, sigma = load_stats(npz)

    o64 = {n: fx.stats(fx.oracle_features(sd, imgs, torch.float64)) for n, imgs in (("real", real), ("gen", gen))}
    o32 = {n: fx.stats(fx.oracle_features(sd, imgs, torch.float32)) for n, imgs in (("real", real), ("gen", gen))}
    rmu, rs = o64["real"]
    emu, es = np.abs(mu - rmu).max() / np.abs(rmu).max(), np.abs(sigma - rs).max() / np.abs(rs).max()
    ymu = 8 * np.abs(o32["real"][0] - rmu).max() / np.abs(rmu).max()
    ys = 8 * np.abs(o32["real"][1] - rs).max() / np.abs(rs).max()
    print(f"e2e mu err {emu:.3e} (yardstick {ymu:.3e}), sigma err {es:.3e} (yardstick {ys:.3e})")
    assert emu <= ymu and es <= ys, (emu, ymu, es, ys)

    want = frechet_distance(*o64["gen"], *o64["real"])
    cpu32 = frechet_distance(*o32["gen"], *o32["real"])
    bound = 2e-5
    assert abs(cpu32 - want) / want <= bound / 8, "fixture: the CPU float32 pipeline is not well inside the bound"
    args = ["--gen_dir", str(gdir), "--dataset", "Toy-48", "--result_dir", str(out)] + extra
    v1 = fid_script.main(args)
    v2 = fid_script.main(args)
    print(f"e2e FID {v1!r} vs oracle {want!r}: rel {abs(v1 - want) / want:.3e} (cpu fp32 {abs(cpu32 - want) / want:.3e})")
    assert want > 0 and abs(v1 - want) / want <= bound, (v1, want)
    lines = (out / "fid.txt").read_text().splitlines()
    assert lines == [f"{gdir} {v1}", f"{gdir} {v2}"] and v1 == v2
