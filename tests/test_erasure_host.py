"""Host logic of the artist-erasure score (pdm/utils/erasure_utils.py, scripts/metrics/artist_erasure.py; no GPU): the prompt
lists, the result path and file-name rules, the baselines that raise, the ESD key rewriting, the pairing of the image files
and the statistics."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest

from pdm.utils import erasure_utils as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ["Monet", "Van Gogh", "Pablo Picasso", "Salvador Dali", "Leonardo Da Vinci"]
# rows of each of the reference's datasets/test_<target>.csv (case_number 0..49)
N_PROMPTS = 50


def _script():
    spec = importlib.util.spec_from_file_location(
        "artist_erasure_host", os.path.join(ROOT, "unlearn-ft_amd", "scripts", "metrics", "artist_erasure.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("target", TARGETS)
def test_prompt_lists_parse(target):
    path = E.default_prompts_csv(target)
    assert path == os.path.join(ROOT, "tests", "golden", "artist_prompts", f"test_{target}.csv")
    prompts = E.read_prompts(path)
    assert len(prompts) == N_PROMPTS
    assert all(isinstance(p, str) and p.strip() for p in prompts)
    assert len(set(prompts)) > N_PROMPTS // 2


def test_prompts_are_utf8_and_keep_commas():
    prompts = E.read_prompts(E.default_prompts_csv("Monet"))
    assert prompts[0] == "Impression, Sunrise by Claude Monet"
    assert prompts[4] == "Rouen Cathedral, West Façade, Sunlight by Claude Monet"
    assert E.read_prompts(E.default_prompts_csv("Van Gogh"))[4] == "Café Terrace at Night by Vincent van Gogh"


def test_prompts_csv_needs_both_columns(tmp_path):
    p = tmp_path / "x.csv"
    p.write_text("case_number,prompt\n0,a cat\n")
    with pytest.raises(ValueError, match="evaluation_seed"):
        E.read_prompts(str(p))


def _args(**kw):
    base = dict(result_dir=None, seed=0, res_path="results/results_seed_0/stable-diffusion/",
                model_id="stabilityai/stable-diffusion-2-1", target="Van Gogh", baseline="pdm", ckpt_name=None,
                original_ckpt=None)
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.mark.parametrize("slash", ["", "/"])
def test_result_path_hub_style_model(slash):
    a = _args(ckpt_name="/data/logs/bilevel_vg/checkpoint-300" + slash, original_ckpt="/data/pruned/run7/checkpoint-20000/", seed=3)
    assert E.images_dir(a) == ("results/results_seed_3/stable-diffusion/stabilityai/stable-diffusion-2-1/Van Gogh/pdm/"
                               "benchmarking/concept_erase/bilevel_vg/checkpoint-300/concept_erase")
    assert E.score_file_name(a.ckpt_name) == "clip_scores_checkpoint-300_VG.json"


@pytest.mark.parametrize("slash", ["", "/"])
def test_result_path_local_model_and_result_dir(tmp_path, slash):
    snap = tmp_path / "snapshots" / "sd21"
    snap.mkdir(parents=True)
    out = str(tmp_path / "out")
    a = _args(model_id=str(snap) + slash, result_dir=out, baseline="pruned_baseline", target="Monet",
              original_ckpt="/data/pruned/run7/checkpoint-20000" + slash)
    assert E.images_dir(a) == os.path.join(out, "sd21", "Monet", "pruned_baseline", "benchmarking", "concept_erase", "run7",
                                           "checkpoint-20000", "concept_erase")
    # no ckpt_name: the reference's file name
    assert E.score_file_name(None) == "clip_scores_concept-prune_VG.json"


def test_file_name_of_an_erasure_checkpoint_file():
    name = "models/esd-vangogh_from_vangogh-xattn_1-epochs_1000.pt"
    assert E.score_file_name(name) == "clip_scores_esd-vangogh_from_vangogh-xattn_1-epochs_1000_VG.json"
    assert E.run_ckpt(name, "/x/y/z/") == "models/esd-vangogh_from_vangogh-xattn_1-epochs_1000.pt"
    assert E.run_ckpt(None, "/x/y/z/") == "y/z"
    assert E.result_root(None, 7, "results/results_seed_0/sd-exp/") == "results/results_seed_7/sd-exp"
    assert E.result_root("/r", 7, "results/results_seed_0/sd-exp/") == "/r"


@pytest.mark.parametrize("baseline", ["concept-prune", "concept-ablation", "baseline"])
def test_unbuilt_baselines_raise(baseline, tmp_path):
    with pytest.raises(NotImplementedError, match=baseline):
        E.check_baseline(baseline)
    # and from the script, before anything is created or the GPU is touched
    with pytest.raises(NotImplementedError, match=baseline):
        _script().main(["--target", "Monet", "--baseline", baseline, "--original_ckpt", "/a/b/c/",
                        "--result_dir", str(tmp_path / "r")])
    assert not (tmp_path / "r").exists()


def test_built_baselines_pass_and_unknown_raises():
    for b in ("pdm", "pruned_baseline", "esd", "uce"):
        E.check_baseline(b)
    with pytest.raises(ValueError, match="nonsense"):
        E.check_baseline("nonsense")


def test_script_flags():
    a = _script().parse_args([])
    assert (a.seed, a.hook_module, a.num_inference_steps, a.clip_model, a.gpu) == (0, "unet", 50, "openai/clip-vit-base-patch32", 0)
    assert a.res_path == "results/results_seed_0/stable-diffusion/"
    for name in ("target", "baseline", "ckpt_name", "original_ckpt", "model_id", "base_config_path", "prompts_csv", "result_dir",
                 "tokenizer", "image_resolution", "mixed_precision", "tiny", "batch_size"):
        assert hasattr(a, name), name


def test_esd_key_rewriting():
    w, b, w2 = object(), object(), object()
    nested = {"unet.down_blocks.0.resnets.0.conv1": {"weight": w, "bias": b},
              "unet.mid_block.attentions.0.transformer_blocks.0.attn2.to_k": {"weight": w2}}
    flat = E.esd_state_dict(nested)
    assert flat == {"down_blocks.0.resnets.0.conv1.weight": w, "down_blocks.0.resnets.0.conv1.bias": b,
                    "mid_block.attentions.0.transformer_blocks.0.attn2.to_k.weight": w2}
    assert E.erasure_dir_name("/models/esd-x.y/w.pt") == "_models_esd-x_y_w_pt"


def test_missing_pair_member_raises_with_counts(tmp_path):
    d = tmp_path / "concept_erase"
    d.mkdir()
    for i in range(4):
        (d / f"original_{i}.jpg").write_bytes(b"x")
        if i != 2:
            (d / f"removal_{i}.png").write_bytes(b"x")
    (d / "clip_scores_checkpoint-4_VG.json").write_text("{}")
    with pytest.raises(ValueError, match="4 prompts, 4 original and 3 removal images"):
        E.pair_files(str(d), 4)
    pairs = E.pair_files(str(d), 2)
    assert [tuple(os.path.basename(p) for p in pr) for pr in pairs] == [("original_0.jpg", "removal_0.png"),
                                                                        ("original_1.jpg", "removal_1.png")]
    with pytest.raises(ValueError, match="5 prompts, 4 original and 3 removal images"):
        E.pair_files(str(d), 5)


def test_statistics_equal_numpy():
    sim = [0.31, 0.275, 0.4012, 0.19, 0.2999, 0.333, 0.28]
    flags = [1, 0, 1, 1, 0, 1, 1]
    r = E.statistics(sim, flags)
    assert set(r) == {"avg_similarity", "avg_score", "std_similarity", "std_score"}
    assert r["avg_similarity"] == np.mean(sim) and r["std_similarity"] == np.std(sim)
    assert r["avg_score"] == np.mean(flags) and r["std_score"] == np.std(flags)
    assert all(type(v) is float for v in r.values())
    # fp32 inputs (what the device hands back) are taken as the Python floats they convert to
    s32 = np.asarray(sim, np.float32)
    assert E.statistics(s32.tolist(), flags)["avg_similarity"] == np.mean([float(v) for v in s32])
