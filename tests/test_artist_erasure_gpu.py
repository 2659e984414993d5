"""scripts/metrics/artist_erasure.py (-m gpu): the scoring stage against transformers' numbers
(tests/golden/artist_erasure_hf.npz, tools/make_erasure_golden.py), the whole script on the tiny topology, and the overlay of
erasure checkpoints (UNet2DConditionModelPruned.overlay_state_dict, generate_fid_images.py --erasure_ckpt_path)."""
import csv
import importlib.util
import json
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")

import numpy as np
import pytest
import torch
import yaml

import clip_score_fixtures as fx
import test_fid_images_gpu as fid_test            # its fixture tree and 2-step training run (_setup)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "artist_erasure_hf.npz"))
HEADER = ["", "Unnamed: 0", "case_number", "prompt", "evaluation_seed", "artists", "evaluation_guidance", "base"]
N = 8
PAIR_TOL = 1e-3          # per cosine: the bound of tests/test_clip_score_gpu.py::test_score_and_result_line


def _script(name="artist_erasure"):
    spec = importlib.util.spec_from_file_location(name + "_gpu", os.path.join(ROOT, "unlearn-ft_amd", "scripts", "metrics",
                                                                               name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_csv(path, prompts):
    with open(path, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(HEADER)
        for i, p in enumerate(prompts):
            w.writerow([i, i, i, p, 1000 + i, "Nobody", 7.5, "thing"])
    return path


# ---------------------------------------------------------------------------------------------- 1. scoring
@pytest.fixture(scope="module")
def scoring(tmp_path_factory):
    """The 16 seeded images of the golden as lossless PNGs in the directory the script derives, the captions as a CSV."""
    from PIL import Image
    from pdm.utils import erasure_utils as E
    root = str(tmp_path_factory.mktemp("erasure_score"))
    argv = ["--target", "Nobody", "--baseline", "pdm", "--ckpt_name", os.path.join(root, "runs", "bilevel", "checkpoint-9"),
            "--result_dir", os.path.join(root, "res"), "--model_id", "stabilityai/stable-diffusion-2-1",
            "--prompts_csv", _write_csv(os.path.join(root, "test_Nobody.csv"), fx.E2E_CAPTIONS[:N]),
            "--clip_model", fx.write_hf_dir(root, "tiny"), "--tokenizer", fx.write_tokenizer(os.path.join(root, "tok"))]
    mod = _script()
    d = E.images_dir(mod.parse_args(argv))
    os.makedirs(d)
    for i in range(N):
        Image.fromarray(fx.image_array(64, 64, 2015 + i)).save(os.path.join(d, f"original_{i}.png"))
        Image.fromarray(fx.image_array(64, 64, 2023 + i)).save(os.path.join(d, f"removal_{i}.png"))
    return dict(mod=mod, argv=argv, dir=d, root=root)


def test_pairs_match_transformers(dev, scoring):
    from pdm.models.clip.clip_model import CLIPModel
    from pdm.utils import clip_utils, erasure_utils as E
    a = scoring["mod"].parse_args(scoring["argv"])
    model = CLIPModel.from_pretrained(a.clip_model, device=dev)
    tok = clip_utils.load_tokenizer(a.tokenizer)
    pairs = E.pair_files(scoring["dir"], N)
    so, sr, flags = E.score_pairs(fx.E2E_CAPTIONS[:N], pairs, model, tok, batch_size=3)
    eo, er = np.abs(so - GOLD["sim_orig"]).max(), np.abs(sr - GOLD["sim_removed"]).max()
    print(f"max |cos - transformers|: originals {eo:.2e}, removals {er:.2e}")
    assert so.dtype == np.float32 and sr.dtype == np.float32
    assert eo <= PAIR_TOL and er <= PAIR_TOL
    assert flags.tolist() == GOLD["score"].tolist()
    assert np.array_equal(flags, (sr < so).astype(np.int64))


def test_scoring_stage_json_and_batch_sizes(dev, scoring):
    mod, d = scoring["mod"], scoring["dir"]
    before = sorted(os.listdir(d))
    results = {}
    for bs in (1, 3, 64):
        r = mod.main(scoring["argv"] + ["--batch_size", str(bs)])
        with open(os.path.join(d, "clip_scores_checkpoint-9_VG.json")) as f:
            text = f.read()
        assert json.loads(text) == r
        results[bs] = text
    print(results[64])
    r = json.loads(results[64])
    assert set(r) == {"avg_similarity", "avg_score", "std_similarity", "std_score"}
    assert abs(r["avg_similarity"] - float(GOLD["avg_similarity"])) <= PAIR_TOL
    assert abs(r["std_similarity"] - float(GOLD["std_similarity"])) <= PAIR_TOL
    assert r["avg_score"] == float(GOLD["avg_score"]) and r["std_score"] == float(GOLD["std_score"])
    assert results[1] == results[3] == results[64]
    assert sorted(os.listdir(d)) == sorted(set(before) | {"clip_scores_checkpoint-9_VG.json"})      # nothing was generated


def test_scoring_missing_member_raises(dev, scoring, tmp_path):
    import shutil
    from pdm.utils import erasure_utils as E
    sub = str(tmp_path / "concept_erase")
    shutil.copytree(scoring["dir"], sub)
    os.remove(os.path.join(sub, "removal_5.png"))
    a = scoring["mod"].parse_args(scoring["argv"])
    with pytest.raises(ValueError, match="8 prompts, 8 original and 7 removal images"):
        E.score(fx.E2E_CAPTIONS[:N], sub, a.clip_model, tokenizer=a.tokenizer, device=dev)


def test_hub_id_clip_model_raises(dev, scoring):
    argv = [x for x in scoring["argv"]]
    argv[argv.index("--clip_model") + 1] = "openai/clip-vit-base-patch32"
    with pytest.raises(FileNotFoundError):
        scoring["mod"].main(argv)


# ---------------------------------------------------------------------------------------------- 2. the whole script, tiny
PROMPTS = ["a red thing by the painter", "the blue one of the fifth", "and the fourth by the painter"]


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """checkpoint-2 (original) of the FID-image test's 2-step run, continued to checkpoint-4 (erased) with lr 1e-4."""
    from pdm.training.trainer import UnetFineTuner
    from pdm.utils.config import Cfg
    tmp = tmp_path_factory.mktemp("erasure_e2e")
    path, ck2, snap = fid_test._setup(tmp, bs=2)
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["training"]["max_train_steps"] = 4
    cfg["training"]["optim"]["prediction_model_learning_rate"] = 1e-4
    cfg["training"]["logging"]["resume_from_checkpoint"] = ck2
    UnetFineTuner(Cfg.wrap(cfg)).train()
    ck4 = os.path.join(os.path.dirname(ck2), "checkpoint-4")
    assert os.path.isdir(os.path.join(ck4, "unet"))
    root = str(tmp)
    return dict(root=root, yaml=path, ck2=ck2, ck4=ck4, snap=snap, clip=fx.write_hf_dir(root, "tiny"),
                csv=_write_csv(os.path.join(root, "test_Painter.csv"), PROMPTS))


def _e2e_argv(t, baseline, ckpt_name):
    argv = ["--target", "Painter", "--baseline", baseline, "--base_config_path", t["yaml"], "--model_id", t["snap"],
            "--original_ckpt", t["ck2"] + "/", "--result_dir", os.path.join(t["root"], "res"), "--prompts_csv", t["csv"],
            "--clip_model", t["clip"], "--image_resolution", "64", "--num_inference_steps", "3", "--tiny", "--seed", "0"]
    return argv + (["--ckpt_name", ckpt_name] if ckpt_name else [])


def _jpgs(d):
    out = {}
    for n in sorted(os.listdir(d)):
        if n.endswith(".jpg"):
            with open(os.path.join(d, n), "rb") as f:
                out[n] = f.read()
    return out


def test_whole_script_pdm(dev, trained):
    from PIL import Image
    from pdm.utils import erasure_utils as E
    mod = _script()
    argv = _e2e_argv(trained, "pdm", trained["ck4"] + "/")
    d = E.images_dir(mod.parse_args(argv))
    assert d == os.path.join(trained["root"], "res", "snapshot", "Painter", "pdm", "benchmarking", "concept_erase", "logs",
                             "checkpoint-4", "concept_erase")
    r1 = mod.main(argv)
    names = [f"{k}_{i}.jpg" for k in ("original", "removal") for i in range(3)]
    assert sorted(os.listdir(d)) == sorted(names + ["clip_scores_checkpoint-4_VG.json"])
    for n in names:
        with Image.open(os.path.join(d, n)) as im:
            assert im.size == (64, 64) and im.mode == "RGB" and im.format == "JPEG"
    with open(os.path.join(d, "clip_scores_checkpoint-4_VG.json")) as f:
        text = f.read()
    assert list(json.loads(text)) == ["avg_similarity", "avg_score", "std_similarity", "std_score"] and json.loads(text) == r1
    assert all(np.isfinite(v) for v in r1.values()) and r1["avg_score"] in (0.0, 1 / 3, 2 / 3, 1.0)
    files = _jpgs(d)
    assert any(files[f"original_{i}.jpg"] != files[f"removal_{i}.jpg"] for i in range(3))     # two more steps changed the model
    assert len({files[f"original_{i}.jpg"] for i in range(3)}) == 3                            # the prompts matter
    # a second run scores the files that are there: nothing is generated again
    mtimes = {n: os.stat(os.path.join(d, n)).st_mtime_ns for n in names}
    r2 = mod.main(argv)
    assert {n: os.stat(os.path.join(d, n)).st_mtime_ns for n in names} == mtimes
    assert r2 == r1
    with open(os.path.join(d, "clip_scores_checkpoint-4_VG.json")) as f:
        assert f.read() == text


def test_whole_script_pruned_baseline(dev, trained):
    from pdm.utils import erasure_utils as E
    mod = _script()
    argv = _e2e_argv(trained, "pruned_baseline", None)
    d = E.images_dir(mod.parse_args(argv))
    assert d.endswith(os.path.join("pruned_baseline", "benchmarking", "concept_erase", "logs", "checkpoint-2", "concept_erase"))
    r = mod.main(argv)
    files = _jpgs(d)
    assert sorted(files) == sorted(f"{k}_{i}.jpg" for k in ("original", "removal") for i in range(3))
    for i in range(3):
        assert files[f"removal_{i}.jpg"] == files[f"original_{i}.jpg"], i        # equal latents in, the same model
    assert r["avg_score"] == 0.0 and r["std_score"] == 0.0                         # the comparison is strict
    assert os.path.exists(os.path.join(d, "clip_scores_concept-prune_VG.json"))   # no ckpt_name: the reference's name


# ---------------------------------------------------------------------------------------------- 3. overlay
def _student(dev):
    from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    cfg = UNetConfig.tiny()
    av = arch_vector_for_budget(cfg, 0.6, hw=16)[0]
    return UNet2DConditionModelPruned(cfg, av, dev, torch.bfloat16, train=False, seed=0)


def _esd_dict(sd, seed=0):
    """An ESD-style nested dict for one bias-free attention projection and one conv with a bias, `unet.` in front."""
    g = torch.Generator().manual_seed(seed)
    attn = next(n for n in sd if n.endswith("attn2.to_k.weight"))[:-len(".weight")]
    conv = next(n for n in sd if n.endswith("resnets.0.conv1.weight"))[:-len(".weight")]
    assert attn + ".bias" not in sd and conv + ".bias" in sd
    nested = {"unet." + attn: {"weight": torch.randn(sd[attn + ".weight"].shape, generator=g)},
              "unet." + conv: {"weight": torch.randn(sd[conv + ".weight"].shape, generator=g) * 0.1,
                               "bias": torch.randn(sd[conv + ".bias"].shape, generator=g)}}
    return nested, [attn + ".weight", conv + ".weight", conv + ".bias"]


def test_overlay_changes_only_the_named_tensors(dev, tmp_path):
    from pdm.utils import erasure_utils as E
    unet = _student(dev)
    before = {n: v.clone() for n, v in unet.state_dict().items()}
    nested, names = _esd_dict(before)
    nested["unet.not.a.module"] = {"weight": torch.zeros(3)}                  # unknown keys are ignored (strict=False)
    path = str(tmp_path / "esd-painter.pt")
    torch.save(nested, path)
    E.load_erasure_checkpoint(unet, path)
    after = unet.state_dict()
    assert list(after) == list(before)
    flat = E.esd_state_dict(nested)
    for n in before:
        if n in names:
            assert torch.equal(after[n], flat[n]) and not torch.equal(after[n], before[n]), n
        else:
            assert torch.equal(after[n], before[n]), n
    # a full state dict (no 'esd' in the path) loads strictly
    full = {n: v + 1 for n, v in before.items()}
    path = str(tmp_path / "uce-painter.pt")
    torch.save(full, path)
    E.load_erasure_checkpoint(unet, path)
    assert all(torch.equal(v, full[n]) for n, v in unet.state_dict().items())
    torch.save({n: v for n, v in list(full.items())[1:]}, path)
    with pytest.raises(KeyError):
        E.load_erasure_checkpoint(unet, path)


def test_overlay_wrong_shape_raises(dev):
    unet = _student(dev)
    sd = unet.state_dict()
    name = next(n for n in sd if n.endswith("attn2.to_k.weight"))
    with pytest.raises(ValueError, match="to_k.weight"):
        unet.overlay_state_dict({name: torch.zeros(sd[name].shape[0] + 1, sd[name].shape[1])})
    assert all(torch.equal(v, sd[n]) for n, v in unet.state_dict().items())    # nothing was written


def test_generate_fid_images_with_erasure_checkpoint(dev, trained, tmp_path, monkeypatch):
    from safetensors.torch import load_file
    m = fid_test._script()
    argv = fid_test._argv(trained["yaml"], trained["ck2"], trained["snap"])
    monkeypatch.setattr(sys, "argv", argv)
    m.main()
    plain = fid_test._files(os.path.join(trained["ck2"], "None_fid_images_3"))
    sd = load_file(os.path.join(trained["ck2"], "unet", "diffusion_pytorch_model.safetensors"))
    nested, _ = _esd_dict(sd, seed=1)
    path = str(tmp_path / "models" / "esd-painter.v1.pt")
    os.makedirs(os.path.dirname(path))
    torch.save(nested, path)
    monkeypatch.setattr(sys, "argv", argv + ["--erasure_ckpt_path", path])
    m.main()
    out = os.path.join(trained["ck2"], path.replace("/", "_").replace(".", "_"), "None_fid_images")
    erased = fid_test._files(out)
    assert sorted(erased) == sorted(plain) and len(plain) == 5
    for a in erased.values():
        assert a.shape == (64, 64, 3) and a.dtype == np.uint8
    assert any(not np.array_equal(erased[n], plain[n]) for n in plain)
    assert fid_test._files(os.path.join(trained["ck2"], "None_fid_images_3")).keys() == plain.keys()
