"""Concept algebra and debias-VL in StableDiffusionPruningPipeline.generate_samples and in their two scripts (-m gpu), on the
tiny pipeline of tests/test_plms_step_gpu.py and the tiny checkpoint tree of tests/data_fixtures.py: the captured 5B loop
bit-identical to the eager one, a call without the keyword bit-identical to the same call before any 5B loop existed,
debias-VL's transformed embeddings through the pipeline, and the scripts' files."""
import csv
import importlib.util
import os

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")

import numpy as np
import pytest
import torch

import clip_score_fixtures as cfx
import data_fixtures
import test_plms_step_gpu as plms_test            # its tiny pipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 13
TEXTS = {0: "a red thing", 1: "the blue one", 2: "and a third", 5: "never sampled"}


def _pipe(dev, dtype, kind):
    from pdm.pipelines.pruning_pipelines import DDIMScheduler
    pipe = plms_test._tiny_pipe(dev, dtype)
    if kind == "ddim":
        pipe.scheduler = DDIMScheduler(prediction_type="v_prediction")
    return pipe


def _batch(pipe, B, gen, steps):
    ctx = pipe.unet.cfg.cross_attention_dim
    return dict(prompt_embeds=torch.randn(B, T, ctx, generator=gen), negative_prompt_embeds=torch.randn(B, T, ctx, generator=gen),
                latents=torch.randn(B, 4, 16, 16, generator=gen), num_inference_steps=steps)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_captured_algebra_loop_equals_eager(dev, kind, B, dtype):
    pipe = _pipe(dev, dtype, kind)
    gen = torch.Generator().manual_seed(B)
    ctx = pipe.unet.cfg.cross_attention_dim
    for steps in (1, 4):                                  # PNDM: 2 and 5 U-Net calls, the repeated first call among them
        before = pipe.captures
        for batch in range(2):                            # the second batch replays the first one's capture
            kw = dict(_batch(pipe, B, gen, steps), algebra_embeds=torch.randn(3, T, ctx, generator=gen))
            for out in ("latent", "pt"):
                e = pipe(graph=False, output_type=out, **kw).images
                c = pipe(graph=True, output_type=out, **kw).images
                assert torch.equal(e, c) and torch.isfinite(c).all(), (steps, batch, out)
        assert pipe.captures == before + 1, "one capture per key, reused by the next batch"
        assert list(pipe._loops)[-1][-1] == "algebra"


@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_without_the_keyword_nothing_changes(dev, kind):
    pipe = _pipe(dev, torch.bfloat16, kind)
    gen = torch.Generator().manual_seed(7)
    ctx = pipe.unet.cfg.cross_attention_dim
    kw = dict(_batch(pipe, 2, gen, 3), output_type="latent")
    concepts = torch.randn(3, T, ctx, generator=gen)
    for graph in (True, False):
        plain = pipe(graph=graph, **kw).images
        captures, keys = pipe.captures, list(pipe._loops)
        if graph:
            assert captures == 1 and "algebra" not in keys[-1]
        on = pipe(graph=graph, algebra_embeds=concepts, **kw).images
        assert torch.isfinite(on).all() and not torch.equal(on, plain)
        assert pipe.captures == captures + int(graph)
        again = pipe(graph=graph, **kw).images           # after a 5B loop exists: the plain call's own loop, same bits
        assert torch.equal(again, plain) and pipe.captures == captures + int(graph)
        if graph:
            assert sorted(map(str, pipe._loops)) == sorted(map(str, keys + [keys[-1] + ("algebra",)]))
    # equal concepts p0 == p1: the projection is left out (the reference samples NaN there); both loops agree and stay finite
    same = torch.cat([concepts[:1], concepts[:1], concepts[2:]])
    c, e = pipe(graph=True, algebra_embeds=same, **kw).images, pipe(graph=False, algebra_embeds=same, **kw).images
    assert torch.equal(c, e) and torch.isfinite(c).all()


def test_end_iteration_and_embedding_shapes(dev):
    pipe = _pipe(dev, torch.bfloat16, "plms")
    gen = torch.Generator().manual_seed(13)
    ctx = pipe.unet.cfg.cross_attention_dim
    kw = dict(_batch(pipe, 2, gen, 4), output_type="latent")
    concepts = torch.randn(3, T, ctx, generator=gen)
    full = pipe(algebra_embeds=concepts, **kw).images
    for end in (0, 1, 2, 5):                              # U-Net calls: PNDM's repeated call is one of them
        e = pipe(graph=False, end_iteration=end, algebra_embeds=concepts, **kw).images
        c = pipe(graph=True, end_iteration=end, algebra_embeds=concepts, **kw).images
        assert torch.equal(e, c), end
    assert torch.equal(c, full)
    with pytest.raises(ValueError, match="three concepts of shape"):
        pipe(algebra_embeds=torch.randn(3, T + 1, ctx, generator=gen), **kw)


# ---------------------------------------------------------------------------------------------- debias-VL and the scripts
def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_sampling_gpu", os.path.join(
        ROOT, "unlearn-ft_amd", "scripts", "baselines", "unified_concept_editing", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tree(tmp_path_factory, dev):
    from pdm.utils.load_models import FrozenModels, inference_config
    t = data_fixtures.write_pruned_checkpoint_tree(str(tmp_path_factory.mktemp("debias_sampling")), dev, "debias_sampling.yaml")
    prompts = os.path.join(t["root"], "prompts.csv")
    with open(prompts, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["case_number", "prompt", "evaluation_seed"])
        for c, text in TEXTS.items():
            w.writerow([c, text, 1000 + c])
    # an erasure checkpoint: the full state dict with every cross-attention key / value weight scaled
    erased = {n: (v * 0.5 if ("attn2.to_k" in n or "attn2.to_v" in n) else v.clone()) for n, v in t["sd"].items()}
    os.makedirs(os.path.join(t["root"], "models"))
    torch.save(erased, os.path.join(t["root"], "models", "diffusers-erased-thing.pt"))
    models = FrozenModels(inference_config(t["yaml"], t["snap"], tiny=True), dev)
    return dict(t, prompts=prompts, models=models)


def _argv(tree, save, model="original"):
    return ["--model_name", model, "--prompts_path", tree["prompts"], "--save_path", save, "--from_case", "1", "--till_case", "2",
            "--num_samples", "2", "--ddim_steps", "2", "--image_size", "64", "--base_config_path", tree["yaml"],
            "--model_id", tree["snap"], "--ckpt_path", tree["ck"], "--tiny", "--models_dir", os.path.join(tree["root"], "models")]


def _check_files(save, folder_name, written, want):
    """The folder rule, the PNG names of cases 1 and 2 (0 and 5 lie outside --from_case / --till_case) and their pixels."""
    from PIL import Image
    folder = os.path.join(save, folder_name)
    names = [f"{c}_{n}.png" for c in (1, 2) for n in range(2)]
    assert sorted(os.listdir(save)) == [folder_name] and sorted(os.listdir(folder)) == names
    assert written == [os.path.join(folder, n) for n in names]
    for c in (1, 2):
        assert want[c].shape == (2, 64, 64, 3) and not np.array_equal(want[c][0], want[c][1])      # one batch, two noise draws
        for n in range(2):
            with Image.open(os.path.join(folder, f"{c}_{n}.png")) as im:
                assert im.format == "PNG" and im.mode == "RGB" and np.array_equal(np.asarray(im), want[c][n]), (c, n)
    return folder


def _sample(pipe, dev, c, **kw):
    return pipe(generator=torch.Generator(device=dev).manual_seed(1000 + c), num_inference_steps=2, guidance_scale=7.5, height=64,
                width=64, output_type="u8_round", **kw).images


def test_debias_vl_through_the_pipeline(dev, tree):
    from pdm import _pdmk as k
    from pdm.utils import debias_vl as D
    models = tree["models"]
    pipe = models.pipeline(models.load_unet(tree["ck"]))
    concepts = ["Thing", "Blue One"]
    factor = D.calibration(models, concepts)
    assert factor.z.shape == (4, factor.d) and factor.z.dtype == torch.float32 and int(factor.info.item()) == 0
    assert torch.allclose(factor.z.norm(dim=1), torch.ones(4, device=dev), atol=1e-5)
    # z are the normalised EOS rows of the four prompts
    tok = models.tokenizer
    ids = tok(D.build_prompts(concepts), padding="max_length", max_length=tok.model_max_length, truncation=True,
              return_tensors="pt").input_ids
    hidden = models.text_encoder(ids.to(dev))[0].float()
    eos = hidden[torch.arange(4, device=dev), ids.argmax(-1).to(dev)]
    assert torch.allclose(factor.z, eos / eos.norm(dim=1, keepdim=True), atol=1e-6)
    emb = pipe.text_encoder(pipe._tokenize([TEXTS[1]]))[0]
    neg = pipe.text_encoder(pipe._tokenize([""]))[0]
    moved = D.apply(factor, emb)
    assert moved.shape == emb.shape and moved.dtype == emb.dtype and not torch.equal(moved, emb)
    again = D.apply(factor, moved)                        # applies again: same shape and dtype
    assert again.shape == emb.shape and again.dtype == emb.dtype
    # against the fp64 statement P = inv(500 M + I) on the same z
    delta = (factor.z[0::2] - factor.z[1::2]).double().cpu()
    G = 500.0 / 2 * delta.T @ delta + torch.eye(factor.d, dtype=torch.float64)
    want = emb[0].double().cpu() @ torch.linalg.inv(G).T
    assert torch.allclose(moved[0].double().cpu(), want, atol=1e-5)
    lat = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(3))
    kw = dict(latents=lat, num_inference_steps=3, output_type="latent")
    got = pipe(prompt_embeds=moved, negative_prompt_embeds=neg, **kw).images
    # a manual run: the eager loop written out, the transformed embeddings on the conditional rows only
    sch = pipe.scheduler
    sch.set_timesteps(3, device=dev)
    x, ehs = lat.to(dev), torch.cat([neg, moved])
    for t in sch.timesteps.tolist():
        out = pipe.unet(torch.cat([x, x]), torch.full((2,), t, device=dev, dtype=torch.int64), ehs, return_dict=False)[0]
        noise = out[1:]
        k.axpby(out[:1], noise, 1.0 - 7.5, 7.5)
        x = sch.step(noise.contiguous(), t, x, return_dict=False)[0]
    assert torch.equal(got, x) and not torch.equal(got, pipe(prompt_embeds=emb, negative_prompt_embeds=neg, **kw).images)
    assert torch.equal(got, pipe(graph=False, prompt_embeds=moved, negative_prompt_embeds=neg, **kw).images)


def test_concept_algebra_script(dev, tree):
    mod = _script("concept_algebra")
    models = tree["models"]
    save = os.path.join(tree["root"], "calg")
    written = mod.main(_argv(tree, save) + ["--concepts_to_project", "a red thing, the blue one ,a third"])
    pipe = models.pipeline(models.load_unet(tree["ck"]))
    want = {c: _sample(pipe, dev, c, prompt=[TEXTS[c]] * 2, algebra_concepts=["a red thing", "the blue one", "a third"])
            for c in (1, 2)}
    _check_files(save, "original", written, want)
    plain = _sample(pipe, dev, 1, prompt=[TEXTS[1]] * 2)
    assert not np.array_equal(plain, want[1])
    # an erasure checkpoint as --model_name, looked up under --models_dir
    from pdm.utils.erasure_utils import load_erasure_checkpoint
    save2 = os.path.join(tree["root"], "calg_erased")
    written = mod.main(_argv(tree, save2, "diffusers-erased-thing.pt"))
    erased = models.pipeline(load_erasure_checkpoint(models.load_unet(tree["ck"]),
                                                     os.path.join(tree["root"], "models", "diffusers-erased-thing.pt")))
    want2 = {c: _sample(erased, dev, c, prompt=[TEXTS[c]] * 2, algebra_concepts=["a man", "a woman", "a person"]) for c in (1, 2)}
    _check_files(save2, "erased-thing", written, want2)
    with pytest.raises(ValueError, match="3 concepts"):
        mod.main(_argv(tree, save) + ["--concepts_to_project", "a man,a woman"])
    with pytest.raises(FileNotFoundError, match="no-such-edit.pt"):
        mod.main(_argv(tree, save, "no-such-edit.pt"))


def test_debiasing_vl_script_and_clip_classify(dev, tree):
    from pdm.utils import debias_vl as D
    mod = _script("debiasing_vl")
    models = tree["models"]
    save = os.path.join(tree["root"], "dvl")
    written = mod.main(_argv(tree, save, "diffusers-erased-thing.pt") + ["--debias_concepts", "Thing, Blue One"])
    from pdm.utils.erasure_utils import load_erasure_checkpoint
    pipe = models.pipeline(load_erasure_checkpoint(models.load_unet(tree["ck"]),
                                                   os.path.join(tree["root"], "models", "diffusers-erased-thing.pt")))
    factor = D.calibration(models, ["Thing", "Blue One"])
    neg = pipe.text_encoder(pipe._tokenize([""]))[0].expand(2, -1, -1)
    want, changed = {}, False
    for c in (1, 2):
        emb = pipe.text_encoder(pipe._tokenize([TEXTS[c]]))[0]
        want[c] = _sample(pipe, dev, c, prompt_embeds=D.apply(factor, emb).expand(2, -1, -1), negative_prompt_embeds=neg)
        changed = changed or not np.array_equal(want[c], _sample(pipe, dev, c, prompt=[TEXTS[c]] * 2))
    folder = _check_files(save, "erased-thing", written, want)
    assert changed, "the calibration left every pixel of the plain samples unchanged"
    # CLIP_classify.py reads the folder unchanged
    clip_dir = cfx.write_hf_dir(tree["root"], "tiny")
    out = _script("CLIP_classify").main(["--im_path", folder, "--prompts_path", tree["prompts"], "--save_path",
                                         os.path.join(tree["root"], "classified"), "--attributes", "a man, the sea",
                                         "--clip_model", clip_dir])
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert out.endswith("erased-thing_gender_classify.csv") and [r[0] for r in rows[1:]] == ["1", "2"]
    assert all(0.0 <= float(v) <= 1.0 for r in rows[1:] for v in r[3:])
