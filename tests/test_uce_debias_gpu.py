"""UCE debiasing on the GPU (-m gpu), on the tiny tree of data_fixtures.write_pruned_checkpoint_tree with the tiny CLIP directory
and tokenizer of clip_score_fixtures: two consecutive `debias_edit` calls against the fp64 restatement of the reference's
mat1 inverse(mat2) with its aliased running norm (tests/uce_debias_fixtures.py), the device-resident measurement against the
existing host route, `get_ratios` with a bypassed text, `debias_model`'s bookkeeping and its captured sampler, and the two
scripts.

Bounds.  The edit: as tests/test_uce_gpu.py::test_edit_model - no further from the fp64 restatement than its fp32 restatement
is, and the edit moves the weights by at least 100 x that distance.  The measurement: frames, pixel values and hence features
bit for bit those of the host route; masks equal to the restatement's on every row whose fp64 top-2 cosine gap is >= 1e-3, and
at most 1 row in 10 below that gap."""
import csv
import importlib.util
import os

import numpy as np
import pytest
import torch

import clip_score_fixtures as cfx
import data_fixtures
import uce_debias_fixtures as fx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, STEPS = 64, 2
OLD = ["van gogh", "the sea"]
NEW = [["art", "a painter of the"], ["sky", "an old and"]]              # attribute texts of other token lengths
CLASSES = ["a man", "a woman", "the sea"]
FRAME_SEED = 11                  # latents of test_classify_frames: chosen on the first GPU run from the restatement's gaps only


def _bits(t):
    return t.contiguous().view(torch.int32)


def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_debias_gpu", os.path.join(
        ROOT, "unlearn-ft_amd", "scripts", "baselines", "unified_concept_editing", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tree(tmp_path_factory, dev):
    from pdm.models.clip.clip_model import CLIPModel
    from pdm.utils import clip_utils
    from pdm.utils.load_models import FrozenModels, inference_config
    t = data_fixtures.write_pruned_checkpoint_tree(str(tmp_path_factory.mktemp("uce_debias")), dev, "uce_debias.yaml")
    config = inference_config(t["yaml"], t["snap"], tiny=True)
    models = FrozenModels(config, dev)
    clip_dir = cfx.write_hf_dir(t["root"], "tiny")
    clip = CLIPModel.from_pretrained(clip_dir, device=dev)
    return dict(t, config=config, models=models, clip_dir=clip_dir, clip=clip, clip_tok=clip_utils.load_tokenizer(clip_dir))


def _load(tree):
    return tree["models"].load_unet(tree["ck"])


def _is_kv(name):
    return name.endswith(".attn2.to_k.weight") or name.endswith(".attn2.to_v.weight")


def _sample(pipe, dev, out="latent"):
    g = torch.Generator().manual_seed(4)
    pe, ne, lat = (torch.randn(1, data_fixtures.T, 64, generator=g), torch.randn(1, data_fixtures.T, 64, generator=g),
                   torch.randn(1, 4, 16, 16, generator=g))
    im = pipe.generate_samples(prompt_embeds=pe.to(dev), negative_prompt_embeds=ne.to(dev), latents=lat.to(dev),
                               num_inference_steps=3, guidance_scale=7.5, output_type=out).images
    return im.cpu() if out == "latent" else im


# ---------------------------------------------------------------------------------------------- the edit
def _groups(state, windows):
    out = []
    for w in windows:
        so, sn = fx.group_slices(state.count[w.old], [state.count[t] for t in w.news], data_fixtures.T)
        eo = state.emb[w.old].cpu()[so]
        eas = [state.emb[t].cpu()[s] for t, s in zip(w.news, sn)]
        assert all(ea.shape == eo.shape for ea in eas) and eo.shape[0] >= 2
        out.append((eo, eas))
    return out


def _check_edit(tag, before, after, groups, rets, weights, lamb, s_e, s_r):
    kv = [n for n in after if _is_kv(n)]
    assert len(kv) >= 4
    for n, v in after.items():
        if _is_kv(n):
            assert v.dtype == torch.float32 and not torch.equal(v, before[n]), n      # every one of them changed
        else:
            assert v.dtype == before[n].dtype and torch.equal(v, before[n]), n
    ref64 = [fx.reference_debias_edit(before[n], groups, rets, weights, lamb, s_e, s_r, torch.float64) for n in kv]
    ref32 = [fx.reference_debias_edit(before[n], groups, rets, weights, lamb, s_e, s_r, torch.float32) for n in kv]
    d_ref = fx.distance(ref32, ref64)
    d = fx.distance([after[n] for n in kv], ref64)
    moved = fx.distance([before[n] for n in kv], ref64)
    print(f"debias_edit {tag}: d_ref {d_ref:.3e}, edit {d:.3e}, moved {moved:.3e}")
    assert moved >= 100 * d_ref                                       # the check is not empty
    assert d <= d_ref


def test_two_consecutive_edits(dev, tree):
    from pdm.utils import uce_debias as D
    lamb, s_e, s_r = 0.5, 1.0, 0.1
    unet = _load(tree)
    state, windows = D.prepare(tree["models"].text_encoder, tree["models"].tokenizer, OLD, NEW, dev)
    assert len({state.count[t] for t in OLD + NEW[0] + NEW[1]}) >= 3
    groups = _groups(state, windows)
    sd0 = {n: v.clone() for n, v in unet.state_dict().items()}
    assert list(sd0) == list(tree["sd"])

    w1 = [torch.tensor([0.05, -0.03]), torch.tensor([-0.04, 0.02])]
    r1 = ["", "monet"]
    D.debias_edit(unet, state, windows, w1, r1, lamb, s_e, s_r)
    sd1 = {n: v.clone() for n, v in unet.state_dict().items()}
    assert list(sd1) == list(sd0) and state.factorisations == 1
    _check_edit("first", sd0, sd1, groups, [state.emb[t].cpu() for t in r1], w1, lamb, s_e, s_r)

    # other weights, a grown retain list (as np.unique leaves it): the system is factored again, and the values start from
    # the first edit's weights
    w2 = [torch.tensor([-0.02, 0.05]), torch.tensor([0.0, 0.0])]
    r2 = [str(t) for t in np.unique(r1 + ["the sea"])]
    D.debias_edit(unet, state, windows, w2, r2, lamb, s_e, s_r)
    sd2 = unet.state_dict()
    assert state.factorisations == 2
    _check_edit("second", sd1, sd2, groups, [state.emb[t].cpu() for t in r2], w2, lamb, s_e, s_r)

    # the same retain list again: nothing is factored
    D.debias_edit(unet, state, windows, w1, r2, lamb, s_e, s_r)
    assert state.factorisations == 2


def test_edit_raises_before_any_weight_is_touched(dev, tree):
    from pdm.utils import uce_debias as D
    unet = _load(tree)
    state, windows = D.prepare(tree["models"].text_encoder, tree["models"].tokenizer, OLD, NEW, dev)
    with pytest.raises(RuntimeError, match="not positive definite at column 0"):
        D.debias_edit(unet, state, windows, [torch.tensor([0.05, 0.05])] * 2, [""], lamb=-1e6)
    assert all(torch.equal(v, tree["sd"][n]) for n, v in unet.state_dict().items())


# ---------------------------------------------------------------------------------------------- the measurement
def test_classify_frames_against_the_host_route(dev, tree):
    from pdm.utils import clip_utils, uce_debias as D
    clip, B = tree["clip"], 10
    pipe = tree["models"].pipeline(_load(tree))
    emb = pipe.text_encoder(pipe._tokenize(["the sea"]))[0].expand(B, -1, -1)
    neg = pipe.text_encoder(pipe._tokenize([""]))[0].expand(B, -1, -1)
    lat = D.seed_latents(pipe, FRAME_SEED, B, RES).to(dev)
    kw = dict(prompt_embeds=emb, negative_prompt_embeds=neg, latents=lat, num_inference_steps=STEPS, guidance_scale=7.5, height=RES,
              width=RES)
    host = pipe.generate_samples(output_type="u8_round", **kw).images
    frames = D.decode_frames(pipe, pipe.generate_samples(output_type="latent", **kw).images)
    assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (B, RES, RES, 3)
    assert torch.equal(frames.cpu(), torch.from_numpy(host))          # the bytes of output_type="u8_round"
    assert len({bytes(h.tobytes()) for h in host}) == B               # ten different images

    R = clip.image_size
    packed, desc = clip_utils.pack_images(list(host), R)
    pix_host = clip_utils.prep_images(packed, desc, R, dev)
    pix = D.frame_pixels(frames, R)
    assert torch.equal(_bits(pix.cpu()), _bits(pix_host.cpu()))        # hence the features are equal
    feats = clip.encode_image(pix_host)
    classes = clip.encode_text(clip_utils.tokenize(tree["clip_tok"], CLASSES, context_length=clip.context_length))
    group = torch.tensor([0, 1] * (B // 2), dtype=torch.int32).to(dev)
    hits = torch.zeros((2, len(CLASSES)), device=dev, dtype=torch.int32)
    probs, mask = D.classify_frames(clip, frames, classes, group, hits)
    _logits, probs64, mask64, gap = fx.zeroshot(feats.cpu(), classes.cpu(), D.logit_scale(clip))
    ok = gap >= fx.GAP
    print(f"classify_frames: {int(ok.sum())} of {B} rows eligible, smallest gap {float(gap.min()):.2e}, "
          f"winners {mask64.argmax(1).tolist()}")
    assert int(ok.sum()) >= B - B // 10                               # otherwise: unsuitable input
    assert torch.equal(mask.cpu()[ok], mask64[ok])
    if bool(ok.all()):
        want = torch.stack([mask64[0::2].sum(0), mask64[1::2].sum(0)]).to(torch.int32)
        assert torch.equal(hits.cpu(), want)
    assert fx.ulps(probs.cpu().numpy()[ok.numpy()], probs64.numpy()[ok.numpy()]).max() <= 4


def test_get_ratios_bypass(dev, tree):
    from pdm.utils import uce_debias as D
    pipe = tree["models"].pipeline(_load(tree))
    calls = []
    inner = pipe.generate_samples
    pipe.generate_samples = lambda *a, **kw: (calls.append(kw["prompt_embeds"]), inner(*a, **kw))[1]
    prev = [torch.tensor([0.3, 0.7]), None]
    ratios = D.get_ratios(pipe, tree["clip"], tree["clip_tok"], OLD, NEW, [True, False], prev, [5, 6, 7], 2, STEPS, RES)
    assert len(calls) == 3 and pipe.captures == 1                     # three seeds of the one text that is measured, one graph
    want = pipe.text_encoder(pipe._tokenize([OLD[1]]))[0]
    assert all(torch.equal(c[0], want[0]) for c in calls)
    assert ratios[0] is prev[0]
    r = ratios[1]
    assert r.dtype == torch.float32 and tuple(r.shape) == (2,) and float(r.sum()) >= 1
    assert torch.equal(r * 6, (r * 6).round())                         # shares of six images
    first = D.get_ratios(pipe, tree["clip"], tree["clip_tok"], OLD, NEW, None, None, [5, 6, 7], 2, STEPS, RES)
    assert len(calls) == 9 and pipe.captures == 1 and torch.equal(first[1], r)


# ---------------------------------------------------------------------------------------------- the outer loop
def _run_model(tree, dev, seed, record=None):
    from pdm.utils import uce_debias as D
    pipe = tree["models"].pipeline(_load(tree))
    before = _sample(pipe, dev)
    settings = dict(D.load_settings(), max_iterations=2, num_seeds=2, num_inference_steps=STEPS)
    inner = D.get_ratios
    if record is not None:
        D.get_ratios = lambda *a, **kw: (record.append(inner(*a, **kw)), record[-1])[1]
    try:
        out = D.debias_model(pipe, tree["clip"], tree["clip_tok"], OLD, NEW, ["", "monet"], np.random.RandomState(seed),
                             num_images=2, resolution=RES, settings=settings)
    finally:
        D.get_ratios = inner
    return pipe, before, out


def test_debias_model(dev, tree, tmp_path):
    from pdm.utils import uce_debias as D
    measured = []
    pipe, before, (weights, init_ratios, ratios, iterations) = _run_model(tree, dev, 3, measured)
    print(f"debias_model: measured {[[r.tolist() for r in m] for m in measured]}")
    assert iterations == len(measured) == 2
    assert all(torch.equal(a, b) for a, b in zip(init_ratios, measured[0]))
    assert all(torch.equal(a, b) for a, b in zip(ratios, measured[1]))
    s1 = D.schedule(measured[0], None, None, ["", "monet"], OLD)
    assert not s1.done                                                 # otherwise: unsuitable input, nothing was edited
    s2 = D.schedule(measured[1], measured[0], s1.max_change, s1.retain_texts, OLD)
    last = s1 if s2.done else s2
    assert all(torch.equal(a, b) for a, b in zip(weights, last.weights))
    for c, skipped in enumerate(s1.bypass):                            # a bypassed text kept its ratio
        if skipped:
            assert measured[1][c] is measured[0][c]
    sd = pipe.unet.state_dict()
    assert all(torch.equal(v, tree["sd"][n]) != _is_kv(n) for n, v in sd.items())
    # the captured sampler sees the edit, and a model loaded from the saved file samples the same bits
    after = _sample(pipe, dev)
    assert not torch.equal(after, before)
    path = str(tmp_path / "unbiased.pt")
    torch.save(sd, path)
    other = _load(tree)
    other.load_state_dict(torch.load(path, map_location="cpu"))
    assert torch.equal(_bits(_sample(tree["models"].pipeline(other), dev)), _bits(after))
    # the same seed again: the same bits
    pipe2, _b, _o = _run_model(tree, dev, 3)
    sd2 = pipe2.unet.state_dict()
    assert all(torch.equal(_bits(sd2[n].float()), _bits(v.float())) for n, v in sd.items())


# ---------------------------------------------------------------------------------------------- the scripts
def test_train_debias_script(dev, tree):
    from pdm.utils import erasure_utils as E, uce_debias as D
    script = _script("train_debias")
    out_dir = os.path.join(tree["root"], "out")
    settings = dict(D.load_settings(), max_iterations=1, num_seeds=1, num_inference_steps=STEPS)
    base = ["--concept", "Sea", "--attributes", "old, a new", "--base_config_path", tree["yaml"], "--model_id", tree["snap"],
            "--ckpt_path", tree["ck"] + "/", "--output_dir", out_dir, "--num_images", "2", "--image_resolution", str(RES), "--tiny"]
    ckpt = script.main(base + ["--clip_model", tree["clip_dir"]], settings=settings)
    name = "unbiased-sea-attributes-old_a9new-sd_2_1"
    assert ckpt == os.path.join(out_dir, "models", name + ".pt") and os.path.exists(ckpt)
    with open(os.path.join(out_dir, "info", name + ".txt")) as f:
        lines = f.read().split("\n")
    assert len(lines) == 4 and lines[0] == str(["image of Sea", "photo of Sea", "portrait of Sea", "picture of Sea", "Sea"])
    assert all(line.startswith("[tensor(") for line in lines[1:])
    sd = torch.load(ckpt, map_location="cpu")
    assert list(sd) == list(tree["sd"]) and all(v.dtype == tree["sd"][n].dtype for n, v in sd.items())
    assert all(torch.equal(v, tree["sd"][n]) != _is_kv(n) for n, v in sd.items())
    # the checkpoint loads through the existing --baseline uce overlay
    E.check_baseline("uce", ckpt_name=ckpt)
    spec = importlib.util.spec_from_file_location("artist_erasure_debias_gpu", os.path.join(ROOT, "unlearn-ft_amd", "scripts", "metrics",
                                                                                           "artist_erasure.py"))
    erasure = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(erasure)
    a = erasure.parse_args(["--target", "Sea", "--baseline", "uce", "--base_config_path", tree["yaml"], "--model_id", tree["snap"],
                            "--original_ckpt", tree["ck"] + "/", "--ckpt_name", ckpt, "--tiny"])
    original, erased = E.load_pipelines(tree["config"], a, dev)
    got = erased.unet.state_dict()
    assert all(torch.equal(got[n], v) for n, v in sd.items())
    assert all(torch.equal(v, tree["sd"][n]) for n, v in original.unet.state_dict().items())
    with pytest.raises(NotImplementedError, match="only 2.1"):
        script.main(base + ["--clip_model", tree["clip_dir"], "--base", "1.4"], settings=settings)
    with pytest.raises(FileNotFoundError, match="hub downloads are not available"):
        script.main(base + ["--clip_model", "openai/clip-vit-base-patch32"], settings=settings)


def test_clip_classify_script(dev, tree):
    from PIL import Image
    from pdm.utils import clip_utils, uce_debias as D
    script = _script("CLIP_classify")
    clip = tree["clip"]
    folder = os.path.join(tree["root"], "images", "model_x")
    os.makedirs(folder)
    images = {"0_0.png": 301, "0_1.png": 302, "1_0.png": 303, "2_0.png": 304, "10_0.png": 305, "10_1.png": 306}
    for n, seed in images.items():
        Image.fromarray(cfx.image_array(64, 64, seed)).save(os.path.join(folder, n))
    with open(os.path.join(folder, "1_1.png"), "wb") as f:
        f.write(b"not an image")
    Image.fromarray(cfx.image_array(64, 64, 1)).save(os.path.join(folder, "0_2.jpg"))          # not a .png: left out
    prompts = os.path.join(tree["root"], "prompts.csv")
    with open(prompts, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["case_number", "prompt", "evaluation_seed"])
        for c in (0, 1, 2, 3, 10):
            w.writerow([c, f"prompt {c}", 100 + c])
    save = os.path.join(tree["root"], "classified")
    attributes = ["a man", "the sea"]
    path = script.main(["--im_path", folder, "--prompts_path", prompts, "--save_path", save, "--attributes", "a man, the sea",
                        "--clip_model", tree["clip_dir"], "--till_case", "9"])
    assert path == os.path.join(save, "model_x_gender_classify.csv")
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["case_number", "prompt", "evaluation_seed", "a_man_bias", "the_sea_bias"]
    assert [r[0] for r in rows[1:]] == ["0", "1", "2"]                 # case 3 has no images, case 10 lies past --till_case
    # the means, from the restatement on the features of the host route, file by file
    classes = clip.encode_text(clip_utils.tokenize(tree["clip_tok"], attributes, context_length=clip.context_length)).cpu()
    masks = {}
    for n in images:
        packed, desc = clip_utils.pack_images([clip_utils.load_image(os.path.join(folder, n))], clip.image_size)
        feat = clip.encode_image(clip_utils.prep_images(packed, desc, clip.image_size, dev)).cpu()
        _l, _p, m, gap = fx.zeroshot(feat, classes, D.logit_scale(clip))
        assert float(gap[0]) >= fx.GAP, (n, float(gap[0]))
        masks[n] = m[0].double()
    want = {0: (masks["0_0.png"] + masks["0_1.png"]) / 2, 1: masks["1_0.png"] / 2, 2: masks["2_0.png"]}
    for r in rows[1:]:
        assert [float(v) for v in r[3:]] == want[int(r[0])].tolist(), r
    with pytest.raises(FileNotFoundError, match="hub downloads are not available"):
        script.main(["--im_path", folder, "--prompts_path", prompts, "--clip_model", "openai/clip-vit-base-patch32"])
