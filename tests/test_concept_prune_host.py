"""ConceptPrune, host side (no GPU): prompt builders, path rules, k / threshold arithmetic, the DDIM scheduler's timesteps and
step coefficients against a float64 restatement of the formulae, from_config strictness, the baseline's name."""
import argparse
import importlib.util
import math
import os
from types import SimpleNamespace

import pytest
import torch

from pdm.pipelines.pruning_pipelines import DDIMScheduler, PNDMScheduler
from pdm.utils import concept_prune as CP
from pdm.utils import erasure_utils as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_cp_host", os.path.join(ROOT, "unlearn-ft_amd", "scripts", "baselines",
                                                                                 "concept_prune", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- prompts
def test_prompts_art():
    base, target = CP.build_prompts("Van Gogh")
    assert len(base) == len(target) == 20
    assert base[0] == "a photo of a cat" and target[0] == "a cat in the style of Van Gogh"
    assert base[-1] == "a photo of a duck" and target[-1] == "a duck in the style of Van Gogh"      # no newline at the file's end


def test_prompts_naked():
    base, target = CP.build_prompts("naked", base="things")          # the word list is `humans`, whatever --base says
    assert len(base) == len(target) == 18
    assert base[0] == "a photo of a man" and target[0] == "a photo of a naked man"
    assert base[2] == "a photo of a girl" and target[2] == "a photo of a naked girl"                 # "girl " in the file
    assert target[16] == "a photo of a naked group of friends"


def test_word_lists_are_the_fixture_files(tmp_path):
    assert CP.read_words(os.path.join(CP.default_words_dir(), "things.txt"))[:3] == ["cat", "dog", "mouse"]
    p = tmp_path / "things.txt"
    p.write_text("one\n\n two words \n")
    assert CP.build_prompts("Monet", words_dir=str(tmp_path)) == (["a photo of a one", "a photo of a two words"],
                                                                  ["a one in the style of Monet", "a two words in the style of Monet"])
    (tmp_path / "empty.txt").write_text("\n")
    with pytest.raises(ValueError):
        CP.read_words(str(tmp_path / "empty.txt"))


@pytest.mark.parametrize("target,kind", [("parachute", "object"), ("female", "gender"), ("memorize_3", "memorize"),
                                         ("coco_memorize", "memorize")])
def test_unbuilt_target_types_raise(target, kind):
    with pytest.raises(NotImplementedError, match=kind):
        CP.build_prompts(target)
    with pytest.raises(ValueError):
        CP.target_type("nobody in particular")


@pytest.mark.parametrize("hook", ["text", "unet-ffn-1", "attn_key", "attn_val"])
def test_unbuilt_hook_modules_raise(hook, tmp_path):
    with pytest.raises(NotImplementedError, match="unet"):
        CP.check_hook_module(hook)
    for name in ("wanda", "save_union_over_time"):          # from the scripts, before anything is created or a GPU is touched
        with pytest.raises(NotImplementedError, match=hook):
            _script(name).main(["--target", "Monet", "--ckpt_path", "/a/b/", "--hook_module", hook, "--result_dir", str(tmp_path / "r")])
    assert not (tmp_path / "r").exists()
    CP.check_hook_module("unet")
    with pytest.raises(ValueError):
        CP.check_hook_module("vae")


# ---- flags, settings and paths
def test_flags_and_settings():
    for name in ("wanda", "save_union_over_time"):
        a = _script(name).parse_args(["--target", "Monet", "--ckpt_path", "/a/b/"])
        assert all(getattr(a, n) is None for n in ("gpu", "dbg", "base", "skill_ratio", "timesteps", "select_ratio", "model_id",
                                                   "base_config_path", "hook_module", "seed", "result_dir", "mixed_precision"))
        assert a.scheduler == "ddim"
        a = CP.resolve_args(a)
        assert (a.gpu, a.base, a.skill_ratio, a.timesteps, a.select_ratio, a.hook_module, a.seed, a.res_path, a.model_id) == \
               (0, "things", 0.01, 50, 0.0, "unet", 43, "results/stable-diffusion", "stabilityai/stable-diffusion-2-1")
        assert a.target == "Monet" and not a.dbg
    a = CP.resolve_args(_script("wanda").parse_args(["--target", "naked", "--ckpt_path", "/a/", "--seed", "7", "--skill_ratio", "0.02"]))
    assert (a.seed, a.skill_ratio) == (7, 0.02)
    with pytest.raises(ValueError):
        CP.resolve_args(_script("wanda").parse_args(["--target", "Monet"]))


def test_path_rules(tmp_path):
    a = SimpleNamespace(hook_module="unet", seed=43, res_path="results/stable-diffusion", result_dir=None,
                        model_id="stabilityai/stable-diffusion-2-1", target="Van Gogh", skill_ratio=0.01)
    p = CP.result_paths(a)
    res = "results/results_seed_43/stable-diffusion/stabilityai/stable-diffusion-2-1/Van Gogh"
    assert p.res_path == res and p.images == res + "/images" and p.skilled_neurons == res + "/skilled_neurons/0.01"
    assert p.checkpoints == res + "/checkpoints"
    assert os.path.join(p.checkpoints, CP.checkpoint_name(0.01, 50, 0.0)) == \
           res + "/checkpoints/skill_ratio_0.01_timesteps_50_threshold0.0.pt"
    snap = tmp_path / "snapshots" / "abc"                   # an existing local path: its basename
    snap.mkdir(parents=True)
    a.model_id, a.result_dir = str(snap), "/r"
    assert CP.result_paths(a).res_path == "/r/abc/Van Gogh"
    a.hook_module = "text"
    with pytest.raises(NotImplementedError):
        CP.result_paths(a)


def test_k_and_threshold():
    assert [CP.top_k(0.01, F) for F in (8, 72, 1000, 1280, 2568, 5120)] == [0, 0, 10, 12, 25, 51]
    assert CP.top_k(1.0, 72) == 72 and CP.top_k(0.25, 72) == 18 and CP.top_k(0.1, 200) == 20
    assert CP.top_k(0.29, 100) == int(0.29 * 100) == 28     # int() of the float product, as the reference
    assert CP.count_threshold(0.0, 50) == 0.0 and CP.count_threshold(0.5, 3) == 1.5
    T = 50
    count = torch.arange(0, T + 1, dtype=torch.int32)
    assert torch.equal(count > CP.count_threshold(0.3, T), count.to(torch.float32) > 0.3 * T)
    assert int((count > CP.count_threshold(0.0, T)).sum()) == T      # 0.0: skilled at one timestep is enough


# ---- DDIM
def _alphas(n=1000, b0=0.00085, b1=0.012):
    betas = torch.linspace(b0 ** 0.5, b1 ** 0.5, n, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).double()


@pytest.mark.parametrize("steps", [1, 3, 50])
def test_ddim_timesteps(steps):
    s = DDIMScheduler()
    s.set_timesteps(steps)
    ratio = 1000 // steps
    assert s.timesteps.tolist() == [i * ratio + 1 for i in reversed(range(steps))]
    assert len(s.timesteps) == steps                        # one U-Net call per step
    p = PNDMScheduler()
    p.set_timesteps(steps)
    assert len(p.timesteps) == (steps + 1 if steps > 1 else len(p.timesteps))


@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_ddim_coefficients(prediction_type):
    """diffusers' DDIM step with eta = 0, restated in float64 on random numbers: x0 and eps from the model output, then
    prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps."""
    steps = 50
    s = DDIMScheduler(prediction_type=prediction_type)
    s.set_timesteps(steps)
    ac = _alphas()
    g = torch.Generator().manual_seed(0)
    x, m = torch.randn(64, dtype=torch.float64, generator=g), torch.randn(64, dtype=torch.float64, generator=g)
    for t in s.timesteps.tolist():
        prev_t = t - 1000 // steps
        a_t = ac[t]
        a_p = ac[prev_t] if prev_t >= 0 else ac[0]
        if prediction_type == "epsilon":
            x0 = (x - (1 - a_t).sqrt() * m) / a_t.sqrt()
            eps = m
        else:
            x0 = a_t.sqrt() * x - (1 - a_t).sqrt() * m
            eps = a_t.sqrt() * m + (1 - a_t).sqrt() * x
        want = a_p.sqrt() * x0 + (1 - a_p).sqrt() * eps
        c_x, c_m = s.coefficients(t)
        assert isinstance(c_x, float) and isinstance(c_m, float)
        assert float((c_x * x + c_m * m - want).abs().max()) <= 1e-12 * (1 + float(want.abs().max()))
    assert s.timesteps[-1] == 1                             # the last step goes to alphas_cumprod[0] (set_alpha_to_one false)
    c_x, c_m = s.coefficients(1)
    assert math.isfinite(c_x) and math.isfinite(c_m)


def test_ddim_from_config_strictness():
    sd21 = {"_class_name": "DDIMScheduler", "_diffusers_version": "0.8.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
            "beta_start": 0.00085, "clip_sample": False, "num_train_timesteps": 1000, "prediction_type": "v_prediction",
            "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None}
    s = DDIMScheduler.from_config(sd21)
    assert s.config.prediction_type == "v_prediction" and s.config.steps_offset == 1
    assert PNDMScheduler.from_config(sd21).config.prediction_type == "v_prediction"      # the same file serves both
    for key, bad in (("beta_schedule", "linear"), ("clip_sample", True), ("set_alpha_to_one", True),
                     ("timestep_spacing", "trailing"), ("trained_betas", [0.1]), ("thresholding", True),
                     ("rescale_betas_zero_snr", True)):
        with pytest.raises(ValueError, match=key):
            DDIMScheduler.from_config({**sd21, key: bad})
    with pytest.raises(ValueError, match="eta_schedule"):
        DDIMScheduler.from_config({**sd21, "eta_schedule": 1})
    with pytest.raises(ValueError, match="prediction_type"):
        DDIMScheduler.from_config({**sd21, "prediction_type": "sample"})


# ---- evaluation hook-up
def test_check_baseline_concept_prune():
    """The baseline is accepted with the checkpoint file it needs; without --ckpt_name (the reference then reads its table of
    checkpoint paths, which is not built) it still raises, as tests/test_erasure_host.py expects of that call."""
    E.check_baseline("concept-prune", ckpt_name="results/x/checkpoints/" + CP.checkpoint_name(0.01, 50, 0.0))
    with pytest.raises(NotImplementedError, match="--ckpt_name"):
        E.check_baseline("concept-prune")
    assert "concept-prune" in E.BASELINES and "concept-prune" not in E.BASELINES_NOT_BUILT
    assert E.score_file_name(None) == "clip_scores_concept-prune_VG.json"
    name = "results/x/checkpoints/" + CP.checkpoint_name(0.01, 50, 0.0)
    assert E.score_file_name(name) == "clip_scores_skill_ratio_0.01_timesteps_50_threshold0.0_VG.json"
