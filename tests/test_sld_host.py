"""Safe Latent Diffusion, host side (no GPU): presets, names, the prompt CSV, the "active" rule and the fp32 rounding of the
scalars (pdm/utils/sld.py, pdm/_pdmk.py sld_params)."""
import argparse
import csv
import ctypes
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = {"Weak": (200, 15, 0.0, 0.0, 0.0), "Medium": (1000, 10, 0.01, 0.3, 0.4), "Strong": (2000, 7, 0.025, 0.5, 0.7),
         "Max": (5000, 0, 1.0, 0.5, 0.7)}


def test_presets_load_from_the_yaml():
    from pdm.utils import sld
    settings = sld.load_settings()
    assert list(settings["presets"]) == list(TABLE)
    for name, want in TABLE.items():
        p = sld.preset(name)
        assert tuple(p[k] for k in sld.PRESET_KEYS) == want, name
        assert isinstance(p["sld_warmup_steps"], int) and all(isinstance(p[k], float) for k in sld.PRESET_KEYS if k != "sld_warmup_steps")
    assert sld.default_concept().startswith("an image showing hate, harassment, violence") and "nudity" in sld.default_concept()
    kw = sld.sampling_kwargs("Strong", "Van Gogh")
    assert kw == dict(sld.preset("Strong"), safety_concept="Van Gogh")
    assert sld.sampling_kwargs("Weak")["safety_concept"] == sld.default_concept()
    for bad in ("medium", "Maximum", "", None):
        with pytest.raises(ValueError, match="sld_type"):
            sld.preset(bad)


def test_settings_file_is_read_not_baked_in(tmp_path):
    import yaml
    from pdm.utils import sld
    settings = sld.load_settings()
    settings["presets"]["Medium"]["sld_threshold"] = 0.5
    path = str(tmp_path / "sld.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(settings, f)
    assert sld.preset("Medium", path)["sld_threshold"] == 0.5
    del settings["presets"]["Max"]["sld_mom_beta"]
    with open(path, "w") as f:
        yaml.safe_dump(settings, f)
    with pytest.raises(ValueError, match="Max"):
        sld.load_settings(path)


def test_directory_and_file_names():
    from pdm.utils import erasure_utils as E, sld
    assert sld.folder_path("out/dir", "Medium", "Van Gogh") == "out/dir/SLD_Medium_Van Gogh"
    assert sld.folder_path("out", "Max", None) == "out/SLD_Max_None"                   # the reference formats None as it is
    assert sld.image_name(38, 2) == "38_2.png"
    assert sld.with_suffix("pruned_baseline", None) == "pruned_baseline"
    assert sld.with_suffix("pruned_baseline", "Max") == "pruned_baseline_SLD_Max"
    args = argparse.Namespace(result_dir="res", seed=0, res_path="results/results_seed_0/stable-diffusion/", model_id="no/such-model",
                              target="Painter", baseline="esd", ckpt_name="runs/esd/esd-painter.pt", original_ckpt=None)
    plain = E.images_dir(args)
    args.sld_type = None
    assert E.images_dir(args) == plain
    args.sld_type = "Weak"
    assert E.images_dir(args) == plain.replace(os.path.join("Painter", "esd"), os.path.join("Painter", "esd_SLD_Weak"))
    assert E.BASELINES == ("pdm", "pruned_baseline", "esd", "uce", "concept-prune")


def test_csv_reading_and_from_case(tmp_path):
    from pdm.utils import erasure_utils as E, sld
    path = str(tmp_path / "prompts.csv")
    with open(path, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", "case_number", "prompt", "evaluation_seed", "artists"])
        for i, (case, prompt, seed) in enumerate([(0, "a, quoted \"one\"", 11), (7, "the second", 4294967295), (3, "third", 5)]):
            w.writerow([i, case, prompt, seed, "Nobody"])
    assert sld.read_cases(path) == [(0, 'a, quoted "one"', 11), (7, "the second", 4294967295), (3, "third", 5)]
    assert sld.read_cases(path, from_case=1) == [(7, "the second", 4294967295), (3, "third", 5)]      # file order, filtered
    assert sld.read_cases(path, from_case=4) == [(7, "the second", 4294967295)]
    assert sld.read_cases(path, from_case=8) == []
    with open(path, "w") as f:
        f.write("prompt,evaluation_seed\nx,1\n")
    with pytest.raises(ValueError, match="case_number"):
        sld.read_cases(path)
    # the shipped artist prompt tables have the three columns
    golden = E.default_prompts_csv("Van Gogh")
    cases = sld.read_cases(golden)
    assert len(cases) == len(E.read_prompts(golden)) and [c[1] for c in cases] == E.read_prompts(golden)


def test_active_rule():
    from pdm.utils import sld
    assert sld.is_active(7.5, 1000, True)
    assert sld.is_active(1.01, 1.01, True)
    assert not sld.is_active(7.5, 1.0, True) and not sld.is_active(7.5, 0.0, True)
    assert not sld.is_active(1.0, 1000, True) and not sld.is_active(0.0, 1000, True)
    assert not sld.is_active(7.5, 1000, False)
    # generate_samples: every SLD keyword defaults to off (no safety concept)
    from pdm.pipelines.pruning_pipelines import StableDiffusionPruningPipeline
    sig = inspect.signature(StableDiffusionPruningPipeline.generate_samples).parameters
    assert all(sig[k].default is None for k in ("safety_concept", "safety_concept_ids", "safety_concept_embeds"))
    assert set(sld.PRESET_KEYS) <= set(sig)


def test_scalars_are_rounded_once_from_doubles():
    from pdm import _pdmk as k
    assert ctypes.sizeof(k.SldParams) == 24
    for name, (scale, warmup, thr, mom, beta) in dict(TABLE, odd=(1234.56789, 3, 0.0123456789, 0.1, 0.9)).items():
        p = k.sld_params(scale, warmup, thr, mom, beta)
        want = [np.float32(scale), np.float32(thr), np.float32(mom), np.float32(beta), np.float32(1.0 - beta)]
        got = [p.sld_guidance_scale, p.threshold, p.momentum_scale, p.mom_beta, p.one_minus_beta]
        assert [np.float32(g) for g in got] == want and all(float(np.float32(g)) == g for g in got), name
        assert p.warmup_steps == warmup and p.key() == tuple(got) + (warmup,)
    # 1 - beta is formed in double: for beta = 0.9 the fp32 difference is another number
    p = k.sld_params(1000, 0, 0.01, 0.3, 0.9)
    assert np.float32(p.one_minus_beta) == np.float32(0.1) != np.float32(1) - np.float32(0.9)
