"""The scripts that sample with Safe Latent Diffusion (-m gpu), on the tiny snapshot and 2-step checkpoint of
tests/test_fid_images_gpu.py: scripts/baselines/unified_concept_editing/sld_generate_images.py, and --sld_type of
scripts/metrics/artist_erasure.py and scripts/metrics/generate_fid_images.py."""
import importlib.util
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")

import numpy as np
import pytest
import torch

import clip_score_fixtures as fx
import test_artist_erasure_gpu as erasure_test    # its CSV writer and argv
import test_fid_images_gpu as fid_test            # its fixture tree and 2-step training run (_setup)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPTS = erasure_test.PROMPTS                    # three rows: case_number i, evaluation_seed 1000 + i


def _sld_script():
    path = os.path.join(ROOT, "unlearn-ft_amd", "scripts", "baselines", "unified_concept_editing", "sld_generate_images.py")
    spec = importlib.util.spec_from_file_location("sld_generate_images_gpu", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sld_scripts")
    path, ck2, snap = fid_test._setup(tmp, bs=2)
    root = str(tmp)
    return dict(root=root, yaml=path, ck2=ck2, snap=snap, clip=fx.write_hf_dir(root, "tiny"),
                csv=erasure_test._write_csv(os.path.join(root, "test_Painter.csv"), PROMPTS))


def _bytes(d):
    return {n: (open(os.path.join(d, n), "rb").read(), os.stat(os.path.join(d, n)).st_mtime_ns) for n in sorted(os.listdir(d))}


def test_sld_generate_images(dev, tree):
    from PIL import Image
    from pdm.utils import sld
    from pdm.utils.load_models import FrozenModels, inference_config
    mod = _sld_script()
    save = os.path.join(tree["root"], "sld_out")
    argv = ["--sld_concept", "Painter", "--sld_type", "Max", "--prompts_path", tree["csv"], "--save_path", save, "--from_case", "1",
            "--num_samples", "2", "--ddim_steps", "3", "--image_size", "64", "--base_config_path", tree["yaml"],
            "--model_id", tree["snap"], "--ckpt_path", tree["ck2"], "--tiny"]
    written = mod.main(argv)
    folder = os.path.join(save, "SLD_Max_Painter")
    names = [f"{case}_{n}.png" for case in (1, 2) for n in range(2)]
    assert sorted(os.listdir(save)) == ["SLD_Max_Painter"] and sorted(os.listdir(folder)) == names
    assert written == [os.path.join(folder, n) for n in names]
    models = FrozenModels(inference_config(tree["yaml"], tree["snap"], True, None), dev)
    pipe = models.pipeline(models.load_unet(tree["ck2"]))
    live = False
    for case in (1, 2):
        kw = dict(prompt=[PROMPTS[case]] * 2, num_inference_steps=3, guidance_scale=7.5, height=64, width=64,
                  output_type="u8_round")
        want = pipe(generator=torch.Generator(device=dev).manual_seed(1000 + case), **kw,
                    **sld.sampling_kwargs("Max", "Painter")).images
        plain = pipe(generator=torch.Generator(device=dev).manual_seed(1000 + case), **kw).images
        live = live or not np.array_equal(want, plain)
        assert want.shape == (2, 64, 64, 3) and not np.array_equal(want[0], want[1])      # one batch, two noise draws
        for n in range(2):
            with Image.open(os.path.join(folder, f"{case}_{n}.png")) as im:
                assert im.format == "PNG" and im.mode == "RGB"
                assert np.array_equal(np.asarray(im), want[n]), (case, n)
    assert live, "SLD Max left every pixel of the plain samples unchanged"
    with pytest.raises(ValueError, match="sld_type"):
        mod.main(argv[:3] + ["Maximum"] + argv[4:])
    assert sorted(os.listdir(save)) == ["SLD_Max_Painter"]


def test_artist_erasure_with_sld(dev, tree):
    from pdm.utils import erasure_utils as E
    mod = erasure_test._script()
    t = dict(tree)
    plain_argv = erasure_test._e2e_argv(t, "pruned_baseline", None)
    plain_dir = E.images_dir(mod.parse_args(plain_argv))
    mod.main(plain_argv)
    before = _bytes(plain_dir)
    argv = plain_argv + ["--sld_type", "Max"]
    d = E.images_dir(mod.parse_args(argv))
    assert d == plain_dir.replace(os.path.join("Painter", "pruned_baseline"), os.path.join("Painter", "pruned_baseline_SLD_Max"))
    r = mod.main(argv)
    assert _bytes(plain_dir) == before, "the plain run's directory is untouched"
    files = erasure_test._jpgs(d)
    assert sorted(files) == sorted(f"{k}_{i}.jpg" for k in ("original", "removal") for i in range(3))
    assert os.path.exists(os.path.join(d, "clip_scores_concept-prune_VG.json")) and all(np.isfinite(v) for v in r.values())
    for i in range(3):                                    # the originals are sampled without SLD
        assert files[f"original_{i}.jpg"] == before[f"original_{i}.jpg"][0], i
    assert any(files[f"removal_{i}.jpg"] != files[f"original_{i}.jpg"] for i in range(3))     # the same model, SLD on
    with pytest.raises(ValueError, match="sld_type"):
        mod.main(plain_argv + ["--sld_type", "max"])


def test_generate_fid_images_with_sld(dev, tree, monkeypatch):
    m = fid_test._script()
    argv = fid_test._argv(tree["yaml"], tree["ck2"], tree["snap"])
    monkeypatch.setattr(sys, "argv", argv)
    m.main()
    plain_dir = os.path.join(tree["ck2"], "None_fid_images_3")
    before = _bytes(plain_dir)
    monkeypatch.setattr(sys, "argv", argv + ["--sld_type", "Weak"])
    m.main()
    out = os.path.join(tree["ck2"], "None_fid_images_3_SLD_Weak")
    got = fid_test._files(out)
    assert sorted(got) == sorted(before) and len(got) == 5
    for a in got.values():
        assert a.shape == (64, 64, 3) and a.dtype == np.uint8
    assert _bytes(plain_dir) == before, "the plain run's directory is untouched"
    monkeypatch.setattr(sys, "argv", argv + ["--sld_type", "Max", "--sld_concept", "a red thing"])
    m.main()
    strong = fid_test._files(os.path.join(tree["ck2"], "None_fid_images_3_SLD_Max"))
    plain = fid_test._files(plain_dir)
    assert sorted(strong) == sorted(plain) and any(not np.array_equal(strong[n], plain[n]) for n in plain)
    assert _bytes(plain_dir) == before
