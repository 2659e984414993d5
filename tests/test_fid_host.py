"""Host side of the FID: the Frechet distance against the scipy TTUR golden, BatchNorm folding, the Inception unit table and
state-dict contract, file listing, statistics files, error paths and the scripts' argument handling.  Runs without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "unlearn-ft_amd", "scripts", "metrics")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fid_frechet.npz")
sys.path.insert(0, SCRIPTS)

from pdm.models import convnet  # noqa: E402
from pdm.models.inception import spec  # noqa: E402
from pdm.utils import fid_utils as fu  # noqa: E402


# ---- Frechet distance
@pytest.mark.parametrize("tag", ["d64", "d256"])
def test_frechet_distance_matches_scipy_golden(tag):
    z = np.load(GOLDEN)
    got = fu.frechet_distance(z[f"{tag}_mu1"], z[f"{tag}_sigma1"], z[f"{tag}_mu2"], z[f"{tag}_sigma2"])
    ref = float(z[f"{tag}_fid"])
    assert abs(got - ref) <= 1e-9 * abs(ref), (got, ref)


def test_frechet_distance_identical_statistics():
    z = np.load(GOLDEN)
    mu, s = z["d256_mu1"], z["d256_sigma1"]
    assert abs(fu.frechet_distance(mu, s, mu, s)) <= 1e-9 * np.trace(s)


def test_frechet_distance_rank_deficient_is_finite():
    g = np.random.default_rng(0)
    a, b = (np.maximum(g.standard_normal((20, 64)) + 0.3, 0) for _ in range(2))      # N = 20 < D = 64
    v = fu.frechet_distance(a.mean(0), np.cov(a, rowvar=False), b.mean(0) + 0.1, np.cov(b, rowvar=False))
    assert np.isfinite(v) and v >= 0


def test_frechet_distance_shape_mismatch():
    with pytest.raises(ValueError):
        fu.frechet_distance(np.zeros(4), np.eye(4), np.zeros(5), np.eye(5))


def test_finish_statistics_matches_numpy():
    g = np.random.default_rng(1)
    f = np.maximum(g.standard_normal((300, 40)) + 0.5, 0).astype(np.float32).astype(np.float64)
    outer = np.triu(f.T @ f)                          # the device fills the upper triangle only
    mu, sigma = fu.finish_statistics(f.sum(0), outer, 300)
    assert np.abs(mu - f.mean(0)).max() <= 1e-13
    assert np.abs(sigma - np.cov(f, rowvar=False)).max() <= 1e-12 * np.abs(sigma).max()
    with pytest.raises(ValueError):
        fu.finish_statistics(f.sum(0), outer, 1)


# ---- BatchNorm folding
@pytest.mark.parametrize("shape,stride,pad", [((8, 5, 3, 3), 2, 0), ((6, 4, 1, 7), 1, (0, 3)), ((7, 3, 1, 1), 1, 0)])
def test_fold_batchnorm_matches_eval_batchnorm(shape, stride, pad):
    g = torch.Generator().manual_seed(0)
    co = shape[0]
    w = torch.randn(*shape, generator=g, dtype=torch.float64)
    gamma, beta, mean = (torch.randn(co, generator=g, dtype=torch.float64) for _ in range(3))
    var = torch.rand(co, generator=g, dtype=torch.float64) + 0.05
    x = torch.randn(2, shape[1], 11, 11, generator=g, dtype=torch.float64)
    ref = F.batch_norm(F.conv2d(x, w, None, stride, pad), mean, var, gamma, beta, False, 0.0, 1e-3)
    wf, bf = convnet.fold_batchnorm(w, gamma, beta, mean, var, spec.BN_EPS)
    got = F.conv2d(x, wf, bf, stride, pad)
    assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()


# ---- the table
def test_unit_table_counts_and_names():
    units = spec.build_units()
    assert len(units) == 94
    assert sum(u.co * u.k + 2 * u.co for u in units) == 21_785_568       # conv weight + BatchNorm weight and bias
    shapes = spec.state_dict_shapes()
    assert len(shapes) == 564
    assert shapes["Conv2d_1a_3x3.conv.weight"] == (32, 3, 3, 3)
    assert shapes["Conv2d_3b_1x1.conv.weight"] == (80, 64, 1, 1)
    assert shapes["Mixed_6b.branch7x7_2.conv.weight"] == (128, 128, 1, 7)
    assert shapes["Mixed_6b.branch7x7dbl_2.conv.weight"] == (128, 128, 7, 1)
    assert shapes["Mixed_6e.branch7x7dbl_5.conv.weight"] == (192, 192, 1, 7)
    assert shapes["Mixed_7a.branch3x3_2.conv.weight"] == (320, 192, 3, 3)
    assert shapes["Mixed_7b.branch3x3_2a.conv.weight"] == (384, 384, 1, 3)
    assert shapes["Mixed_7c.branch3x3dbl_2.conv.weight"] == (384, 448, 3, 3)
    assert shapes["Mixed_7c.branch_pool.bn.running_var"] == (192,)
    assert shapes["Mixed_5b.branch5x5_2.bn.num_batches_tracked"] == ()
    by = {u.name: u for u in units}
    assert (by["Mixed_5b.branch5x5_2"].ph, by["Mixed_5b.branch5x5_2"].pw) == (2, 2)
    assert (by["Mixed_6c.branch7x7_3"].kh, by["Mixed_6c.branch7x7_3"].kw, by["Mixed_6c.branch7x7_3"].ph) == (7, 1, 3)
    assert by["Mixed_6c.branch7x7_1"].co == 160 and by["Mixed_6e.branch7x7_1"].co == 192
    assert by["Mixed_6a.branch3x3"].stride == 2 and by["Conv2d_1a_3x3"].stride == 2


def test_unit_table_shapes_chain():
    """The channel counts the issue lists per stage, from the table alone."""
    by = {u.name: u for u in spec.build_units()}

    def out(block, names):
        return sum(by[f"{block}.{n}"].co for n in names)
    a = ["branch1x1", "branch5x5_2", "branch3x3dbl_3", "branch_pool"]
    assert [out(b, a) for b in ("Mixed_5b", "Mixed_5c", "Mixed_5d")] == [256, 288, 288]
    assert out("Mixed_6a", ["branch3x3", "branch3x3dbl_3"]) + 288 == 768
    assert out("Mixed_6d", ["branch1x1", "branch7x7_3", "branch7x7dbl_5", "branch_pool"]) == 768
    assert out("Mixed_7a", ["branch3x3_2", "branch7x7x3_4"]) + 768 == 1280
    e = ["branch1x1", "branch3x3_2a", "branch3x3_2b", "branch3x3dbl_3a", "branch3x3dbl_3b", "branch_pool"]
    assert out("Mixed_7b", e) == 2048 and out("Mixed_7c", e) == 2048 and by["Mixed_7c.branch1x1"].ci == 2048


def _state_dict():
    sd = spec.init_state_dict(seed=1)
    sd["fc.weight"], sd["fc.bias"] = torch.zeros(1008, 2048), torch.zeros(1008)
    sd["AuxLogits.fc.weight"] = torch.zeros(3)
    return sd


def _checked_trunk(sd):
    """What InceptionV3FID.load_state_dict checks."""
    return convnet.checked(sd, spec.state_dict_shapes(num_batches_tracked=False), "Inception", spec.ignored)


def test_state_dict_contract():
    sd = _state_dict()
    assert len([n for n in sd if not n.startswith(("fc.", "AuxLogits."))]) == 564
    trunk = _checked_trunk(sd)
    assert len(trunk) == 94 * 5 and not any("num_batches_tracked" in n or n.startswith("fc.") for n in trunk)
    missing = dict(sd)
    del missing["Mixed_6c.branch7x7_2.bn.running_mean"]
    with pytest.raises(KeyError, match="Mixed_6c.branch7x7_2.bn.running_mean"):
        _checked_trunk(missing)
    bad = dict(sd)
    bad["Mixed_7a.branch3x3_2.conv.weight"] = torch.zeros(320, 192, 3, 1)
    with pytest.raises(ValueError, match="Mixed_7a.branch3x3_2.conv.weight"):
        _checked_trunk(bad)
    extra = dict(sd)
    extra["Mixed_8a.conv.weight"] = torch.zeros(1)
    with pytest.raises(KeyError):
        _checked_trunk(extra)


def test_from_pretrained_missing_file_names_the_path(tmp_path):
    from pdm.models.inception.inception_v3 import InceptionV3FID, default_weights_path
    assert default_weights_path().endswith(os.path.join(".cache", "torch", "hub", "checkpoints",
                                                        "pt_inception-2015-12-05-6726825d.pth"))
    p = str(tmp_path / "nowhere.pth")
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        InceptionV3FID.from_pretrained(p)


# ---- files, statistics, errors
def test_list_images_sorted_and_filtered(tmp_path):
    (tmp_path / "sub").mkdir()
    for n in ("b.npy", "a.PNG", "c.jpeg", "notes.txt", ".hidden.npy", "sub/d.npy"):
        (tmp_path / n).write_bytes(b"")
    got = [os.path.relpath(p, tmp_path) for p in fu.list_images(str(tmp_path))]
    assert got == ["a.PNG", "b.npy", "c.jpeg", os.path.join("sub", "d.npy")]


def test_stats_path_and_round_trip(tmp_path, monkeypatch):
    p = fu.stats_path("COCO-30k", "legacy_pytorch", str(tmp_path))
    assert p == str(tmp_path / "coco-30k_legacy_pytorch_custom_na.npz")
    monkeypatch.setenv("PDM_FID_STATS", str(tmp_path / "env"))
    assert fu.stats_path("x") == str(tmp_path / "env" / "x_legacy_pytorch_custom_na.npz")
    monkeypatch.delenv("PDM_FID_STATS")
    assert fu.default_stats_dir() == os.path.join(os.path.expanduser("~"), ".cache", "pdm", "fid_stats")
    g = np.random.default_rng(0)
    mu, sigma = g.standard_normal(16), g.standard_normal((16, 16))
    fu.save_stats(p, mu, sigma)
    mu2, sigma2 = fu.load_stats(p)
    assert np.array_equal(mu, mu2) and np.array_equal(sigma, sigma2) and sorted(np.load(p).files) == ["mu", "sigma"]


def test_error_paths(tmp_path):
    with pytest.raises(NotImplementedError, match="clean"):
        fu.compute_fid(str(tmp_path), "coco-30k", mode="clean", stats_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="train"):
        fu.compute_fid(str(tmp_path), "coco-30k", dataset_split="train", stats_dir=str(tmp_path))
    with pytest.raises(NotImplementedError):
        fu.make_custom_stats("x", str(tmp_path), mode="clean", stats_dir=str(tmp_path))
    with pytest.raises(FileNotFoundError) as e:
        fu.compute_fid(str(tmp_path), "coco-30k", stats_dir=str(tmp_path))
    assert "coco-30k_legacy_pytorch_custom_na.npz" in str(e.value) and "make_custom_stats.py" in str(e.value)


def test_pack_images_layout():
    a, b = np.full((2, 3, 3), 7, np.uint8), np.full((1, 1, 3), 9, np.uint8)
    packed, desc = fu.pack_images([a, b])
    assert desc.tolist() == [[0, 2, 3, 2, 3, 0, 0, 0], [20, 1, 1, 1, 1, 0, 0, 0]]
    buf = packed.numpy()
    assert buf[:128].view(np.int64).reshape(2, 8).tolist() == desc.tolist()
    assert (buf[128:146] == 7).all() and (buf[148:151] == 9).all() and packed.numel() == 128 + 24 + 4
    with pytest.raises(ValueError):
        fu.pack_images([np.zeros((2, 2), np.uint8)])


# ---- scripts
def test_fid_script_arguments_and_result_line(tmp_path):
    import fid as fid_script
    a = fid_script.parse_args(["--gen_dir", "g", "--result_dir", "r"])
    assert (a.dataset, a.mode, a.stats_dir, a.inception_weights, a.batch_size, a.num_workers) == \
        ("coco-30k", "legacy_pytorch", None, None, 64, None)
    fid_script.write_result(str(tmp_path / "res"), "/data/gen", 12.5)
    fid_script.write_result(str(tmp_path / "res"), "/data/gen2", 3.25)
    assert (tmp_path / "res" / "fid.txt").read_text() == "/data/gen 12.5\n/data/gen2 3.25\n"


def test_make_custom_stats_script_arguments():
    import make_custom_stats as m
    a = m.parse_args(["--name", "coco-30k", "--data_dir", "d", "--stats_dir", "s", "--batch_size", "8"])
    assert (a.name, a.data_dir, a.mode, a.stats_dir, a.batch_size) == ("coco-30k", "d", "legacy_pytorch", "s", 8)
    with pytest.raises(SystemExit):
        m.parse_args(["--data_dir", "d"])


def test_resize_and_save_images_arguments():
    import resize_and_save_images as rs
    a = rs.parse_args(["--data_dir", "d", "--output_dir", "o"])
    assert a.size == [512, 512]
    a = rs.parse_args(["--data_dir", "d", "--output_dir", "o", "--size", "256", "384"])
    assert tuple(a.size) == (256, 384)
    assert rs.output_name("000000397133.jpg") == "000000397133.npy"
    assert rs.output_name("photo.jpeg") == "photo.npy" and rs.output_name("a.b.webp") == "a.b.npy"
