"""Host side of the two sampling-time debiasing baselines (no GPU): the flags, the three-concept rule and the folder rule of
scripts/baselines/unified_concept_editing/{concept_algebra,debiasing_vl}.py, the male / female prompt builder and the YAML list
of pdm/utils/debias_vl.py, the argument errors of generate_samples' algebra keywords, and that the input recipes of
tests/test_calg_step_gpu.py and tests/test_debias_vl_gpu.py satisfy the conditions those tests rely on."""
import importlib.util
import inspect
import os
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--model_name", "diffusers-erased-Painter.pt", "--prompts_path", "p.csv", "--save_path", "out"]


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_host", os.path.join(
        ROOT, "unlearn-ft_amd", "scripts", "baselines", "unified_concept_editing", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name,flag,default", [("concept_algebra", "concepts_to_project", "a man,a woman,a person"),
                                               ("debiasing_vl", "debias_concepts", "")])
def test_flags_are_the_references(name, flag, default):
    mod = _script(name)
    a = mod.parse_args(COMMON)
    assert (a.device, a.guidance_scale, a.image_size, a.from_case, a.till_case, a.num_samples, a.ddim_steps) == (
        "cuda:0", 7.5, 512, 0, 1000000, 1, 100)
    assert getattr(a, flag) == default
    assert (a.models_dir, a.base_config_path, a.ckpt_path, a.mixed_precision, a.tiny) == ("models", None, None, None, False)
    a = mod.parse_args(COMMON + ["--" + flag, "x, y ,z", "--from_case", "3", "--till_case", "9", "--num_samples", "4",
                                 "--ddim_steps", "20", "--guidance_scale", "3.5", "--image_size", "256", "--tiny",
                                 "--ckpt_path", "ck", "--mixed_precision", "bf16"])
    assert getattr(a, flag) == "x, y ,z" and (a.from_case, a.till_case, a.num_samples, a.ddim_steps) == (3, 9, 4, 20)
    assert (a.guidance_scale, a.image_size, a.tiny, a.ckpt_path, a.mixed_precision) == (3.5, 256, True, "ck", "bf16")
    for missing in ("--model_name", "--prompts_path", "--save_path"):
        argv = list(COMMON)
        i = argv.index(missing)
        with pytest.raises(SystemExit):
            mod.parse_args(argv[:i] + argv[i + 2:])
    with pytest.raises(SystemExit):                       # --base is not offered
        mod.parse_args(COMMON + ["--base", "2.1"])
    for word in ("PNDM", "LMSDiscreteScheduler", "SD-2.1", "SD-1.4", "--base is not offered"):
        assert word in mod.__doc__, word


def test_three_concept_rule():
    from pdm.utils import concept_algebra as A
    assert A.split_concepts(A.DEFAULT_CONCEPTS) == ["a man", "a woman", "a person"]
    assert A.split_concepts(" a doctor ,a nurse, a person ") == ["a doctor", "a nurse", "a person"]
    for bad in ("a man,a woman", "a,b,c,d", "", "one"):
        with pytest.raises(ValueError, match="3 concepts"):
            A.split_concepts(bad)
    mod = _script("concept_algebra")
    with pytest.raises(ValueError, match="3 concepts"):               # before any model is loaded
        mod.main(COMMON + ["--concepts_to_project", "a man,a woman"])
    with pytest.raises(ValueError, match="3 concepts"):
        mod.generate_images(None, "original", "p.csv", ["a", "b"], "out")


def test_folder_paths_and_checkpoint_lookup(tmp_path):
    from pdm.utils import concept_algebra as A
    assert A.folder_path("out", "original") == "out/original"
    assert A.folder_path("out", "diffusers-VanGogh-ESDx1-UNET.pt") == "out/VanGogh-ESDx1-UNET"
    assert A.folder_path("out", "models/unbiased-doctor.pt") == "out/unbiased-doctor"
    assert A.erasure_checkpoint("original", "models") is None
    models = tmp_path / "models"
    models.mkdir()
    (models / "erased.pt").write_bytes(b"x")
    assert A.erasure_checkpoint("erased.pt", str(models)) == os.path.join(str(models), "erased.pt")
    assert A.erasure_checkpoint(str(models / "erased.pt"), "elsewhere") == str(models / "erased.pt")
    with pytest.raises(FileNotFoundError, match="absent.pt"):
        A.erasure_checkpoint("absent.pt", str(models))


def test_prompt_builder_and_yaml_list(tmp_path):
    from pdm.utils import debias_vl as D
    s = D.load_settings()
    assert s["lam"] == 500.0 and len(s["templates"]) == 2
    assert len(s["concepts"]) == 80 and s["concepts"][0] == "Actor" and s["concepts"][-1] == "Zoologist"
    assert "Bus Driver" in s["concepts"] and "DJ" in s["concepts"] and len(set(s["concepts"])) == 80
    assert D.build_prompts(["Bus Driver", "DJ"]) == ["A photo of a male bus driver.", "A photo of a female bus driver.",
                                                     "A photo of a male dj.", "A photo of a female dj."]
    assert D.split_concepts("") == s["concepts"]
    assert D.split_concepts(" Doctor, Nurse ") == ["Doctor", "Nurse"]
    # the file is read, not baked in
    other = tmp_path / "other.yaml"
    other.write_text("lam: 2.0\ntemplates: ['m {}', 'f {}']\nconcepts: [X]\n")
    o = D.load_settings(str(other))
    assert D.build_prompts(["Y z"], o) == ["m y z", "f y z"] and D.split_concepts("", o) == ["X"]
    other.write_text("lam: 2.0\ntemplates: ['m {}']\nconcepts: [X]\n")
    with pytest.raises(ValueError, match="two templates"):
        D.load_settings(str(other))


def _stub_pipe():
    from pdm.pipelines.pruning_pipelines import StableDiffusionPruningPipeline
    vae = SimpleNamespace(cfg=SimpleNamespace(block_out_channels=(1, 1, 1)))
    return StableDiffusionPruningPipeline(vae, None, SimpleNamespace(device=torch.device("cpu")))


def test_generate_samples_argument_errors():
    from pdm.pipelines.pruning_pipelines import StableDiffusionPruningPipeline
    sig = inspect.signature(StableDiffusionPruningPipeline.generate_samples).parameters
    assert all(sig[n].default is None for n in ("algebra_concepts", "algebra_ids", "algebra_embeds"))
    pipe = _stub_pipe()
    e = torch.zeros(1, 5, 8)
    three = torch.zeros(3, 5, 8)
    with pytest.raises(ValueError, match="Safe Latent Diffusion"):
        pipe(prompt_embeds=e, negative_prompt_embeds=e, algebra_embeds=three, safety_concept_embeds=e)
    with pytest.raises(ValueError, match="Safe Latent Diffusion"):
        pipe(prompt_embeds=e, negative_prompt_embeds=e, algebra_concepts=["a", "b", "c"], safety_concept="d")
    for g in (1.0, 0.5):
        with pytest.raises(ValueError, match="guidance_scale"):
            pipe(prompt_embeds=e, negative_prompt_embeds=e, algebra_embeds=three, guidance_scale=g)
    for bad in (dict(algebra_embeds=torch.zeros(2, 5, 8)), dict(algebra_embeds=torch.zeros(4, 5, 8)),
                dict(algebra_ids=torch.zeros(2, 5, dtype=torch.int64)), dict(algebra_concepts=["a", "b"]),
                dict(algebra_concepts="a man"), dict(algebra_concepts=["a", "b", "c", "d"])):
        with pytest.raises(ValueError, match="exactly three"):
            pipe(prompt_embeds=e, negative_prompt_embeds=e, **bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_concept_algebra_recipe_satisfies_its_condition(dtype):
    import test_calg_step_gpu as calg
    for shape, extra in calg.SHAPES:
        have, need = calg.host_condition(shape, extra, dtype)
        print(shape, dtype, "projection term", have, "needed", need)
        assert have >= need


def test_debias_vl_recipe_satisfies_its_condition():
    import test_debias_vl_gpu as vl
    for d, pairs, m in vl.SHAPES:
        z, X, want, d_ref, moved = vl.transform_case(d, pairs, m)
        print(f"d {d} pairs {pairs} m {m}: d_ref {d_ref:.3e}, transform moves X by {moved:.3f}")
        assert torch.allclose(z.norm(dim=1), torch.ones(2 * pairs), atol=1e-6)
        assert d_ref > 0 and moved >= 1000 * 4 * d_ref
