"""Host side of the CLIP score (no GPU): OpenAI -> transformers key mapping and config inference, the two `.pt` formats,
model-name resolution, pairing by stem, caption file naming, token layout, result / feature-directory naming."""
import os
import sys

import numpy as np
import pytest
import torch

import clip_score_fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unlearn-ft_amd", "scripts", "metrics"))


def hf_to_openai(sd):
    """The inverse mapping, written independently of pdm/models/clip/convert.py: q / k / v stacked into in_proj, the
    projections transposed back to x @ P."""
    out = {}
    ren = {"self_attn.out_proj": "attn.out_proj", "layer_norm1": "ln_1", "layer_norm2": "ln_2", "mlp.fc1": "mlp.c_fc",
           "mlp.fc2": "mlp.c_proj"}
    for tower, src in (("visual.", "vision_model."), ("", "text_model.")):
        layers = sorted({int(n.split(".")[3]) for n in sd if n.startswith(src + "encoder.layers.")})
        for i in layers:
            p, q = f"{src}encoder.layers.{i}.", f"{tower}transformer.resblocks.{i}."
            out[q + "attn.in_proj_weight"] = torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
            out[q + "attn.in_proj_bias"] = torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0)
            for a, b in ren.items():
                for s in ("weight", "bias"):
                    out[f"{q}{b}.{s}"] = sd[f"{p}{a}.{s}"]
    out.update({"visual.class_embedding": sd["vision_model.embeddings.class_embedding"],
                "visual.conv1.weight": sd["vision_model.embeddings.patch_embedding.weight"],
                "visual.positional_embedding": sd["vision_model.embeddings.position_embedding.weight"],
                "visual.ln_pre.weight": sd["vision_model.pre_layrnorm.weight"], "visual.ln_pre.bias": sd["vision_model.pre_layrnorm.bias"],
                "visual.ln_post.weight": sd["vision_model.post_layernorm.weight"],
                "visual.ln_post.bias": sd["vision_model.post_layernorm.bias"],
                "visual.proj": sd["visual_projection.weight"].t().contiguous(),
                "token_embedding.weight": sd["text_model.embeddings.token_embedding.weight"],
                "positional_embedding": sd["text_model.embeddings.position_embedding.weight"],
                "ln_final.weight": sd["text_model.final_layer_norm.weight"], "ln_final.bias": sd["text_model.final_layer_norm.bias"],
                "text_projection": sd["text_projection.weight"].t().contiguous(), "logit_scale": sd["logit_scale"]})
    return out


@pytest.mark.parametrize("tag", ["tiny", "b32"])
def test_openai_mapping_and_config_inference(tag):
    from pdm.models.clip import convert
    sd = fx.state_dict(tag)
    osd = hf_to_openai(sd)
    back = convert.openai_to_hf(osd)
    assert set(back) == set(sd)
    for n in sd:
        assert torch.equal(back[n], sd[n]), n
    text, vision, proj = convert.openai_configs(osd)
    t, v, p = fx.CONFIGS[tag]
    assert (text, vision, proj) == (t, v, p)
    with pytest.raises(NotImplementedError):
        convert.openai_configs({"visual.layer1.0.conv1.weight": torch.zeros(1)})


def _script_module(osd):
    """A TorchScript archive holding `osd` under its dotted names, as the clip package's downloads do."""
    root = torch.nn.Module()
    for name, t in osd.items():
        mod, parts = root, name.split(".")
        for part in parts[:-1]:
            if not hasattr(mod, part):
                mod.add_module(part, torch.nn.Module())
            mod = getattr(mod, part)
        mod.register_parameter(parts[-1], torch.nn.Parameter(t.clone(), requires_grad=False))
    root.register_buffer("input_resolution", torch.tensor(224))
    return torch.jit.script(root)


def test_torchscript_and_pickled_pt_load_the_same(tmp_path):
    from pdm.models.clip import convert
    osd = hf_to_openai(fx.state_dict("tiny"))
    a, b = str(tmp_path / "jit.pt"), str(tmp_path / "sd.pt")
    torch.jit.save(_script_module(osd), a)
    torch.save(osd, b)
    ja, pb = convert.load_openai_state_dict(a), convert.load_openai_state_dict(b)
    for n in osd:
        assert torch.equal(ja[n], osd[n]) and torch.equal(pb[n], osd[n]), n
    ta, tb = convert.load_checkpoint(a), convert.load_checkpoint(b)
    assert ta[:3] == tb[:3] == fx.CONFIGS["tiny"]
    assert set(ta[3]) == set(tb[3]) and all(torch.equal(ta[3][n], tb[3][n]) for n in ta[3])


def test_model_name_resolution(tmp_path, monkeypatch):
    from pdm.models.clip import convert
    monkeypatch.setenv("HOME", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="ViT-B-32.pt"):
        convert.resolve("ViT-B/32")
    with pytest.raises(FileNotFoundError):
        convert.resolve("openai/clip-vit-base-patch32")
    with pytest.raises(NotImplementedError):
        convert.resolve("RN50")
    p = tmp_path / ".cache" / "clip" / "ViT-B-32.pt"
    p.parent.mkdir(parents=True)
    p.write_bytes(b"")
    assert convert.resolve("ViT-B/32") == str(p)
    d = fx.write_hf_dir(str(tmp_path), "tiny")
    text, vision, proj, sd = convert.load_checkpoint(d)
    assert (text, vision, proj) == fx.CONFIGS["tiny"] and set(sd) == set(fx.state_dict("tiny"))


def test_pairing_by_stem(tmp_path):
    from pdm.utils.clip_utils import list_dir, pair_by_stem
    t, im = tmp_path / "t", tmp_path / "i"
    t.mkdir()
    im.mkdir()
    for i in range(6):
        np.save(str(t / f"{i:012d}.npy"), np.zeros(4, np.float32))
        np.save(str(im / f"{i:012d}.npy"), np.zeros((2, 2, 3), np.uint8))
    (t / ".hidden").write_text("x")
    tf, imf = list_dir(str(t)), list_dir(str(im))
    pairs = pair_by_stem(tf, imf)
    assert [(a, b) for _, a, b in pairs] == list(zip(tf, imf))           # the reference's sorted pairing, on good dirs
    with pytest.raises(ValueError, match=r"5 images, 6 text features; 0 images without .* 1 text features without an "
                                         r"image \(first: \['000000000002'\]\)"):
        pair_by_stem(tf, [f for f in imf if "000000000002" not in f])
    with pytest.raises(ValueError, match=r"1 images without a text feature \(first: \['extra'\]\)"):
        pair_by_stem(tf, imf + [str(im / "extra.npy")])


def test_save_captions_naming(tmp_path):
    import json
    import save_captions
    for name, want in (("captions_val2014_30k.json", "COCO_val2014_30k_000000000042.txt"),
                       ("captions_val2017.json", "000000000042.txt")):
        d = tmp_path / name.split(".")[0]
        d.mkdir()
        ann = d / name
        ann.write_text(json.dumps({"annotations": [{"image_id": 42, "id": 1, "caption": "first"},
                                                   {"image_id": 42, "id": 2, "caption": "a dog"}]}))
        out = save_captions.main(["--annotations_file", str(ann)])
        assert out == str(d / "clip-captions") and os.listdir(out) == [want]
        assert (d / "clip-captions" / want).read_text() == "a dog"


def test_token_layout_and_overlength(tmp_path):
    from data_fixtures import write_tokenizer
    from pdm.utils.clip_utils import load_tokenizer, tokenize
    tok = load_tokenizer(write_tokenizer(str(tmp_path)))
    ids = tokenize(tok, ["the cat and the dog", "a"], ["x.txt", "y.txt"])
    assert ids.shape == (2, 77) and ids.dtype == torch.int64
    for r in ids:
        n = int((r != 0).sum())
        assert r[0] == fx.VOCAB - 2 and r[n - 1] == fx.VOCAB - 1 and (r[n:] == 0).all()
        assert int(r.argmax()) == n - 1                                   # EOT is the largest id: OpenAI's pooling row
    n0 = int((ids[0] != 0).sum())
    assert n0 > 3 and (ids[0, 1:n0 - 1] < fx.VOCAB - 2).all()
    with pytest.raises(ValueError, match="long.txt"):
        tokenize(tok, ["a b c " * 40], ["long.txt"])
    with pytest.raises(FileNotFoundError, match="--tokenizer"):
        load_tokenizer(str(tmp_path / "nothing"))


def test_result_file_and_feature_dir_naming(tmp_path):
    import clip_score
    from pdm.models.clip.convert import model_tag
    from pdm.utils.clip_utils import features_dir
    assert model_tag("ViT-B/32") == "ViT-B-32"
    assert model_tag("/models/ViT-B-32.pt") == "ViT-B-32"
    assert model_tag("/models/clip-vit-base-patch32/") == "clip-vit-base-patch32"
    assert features_dir("/data/coco/annotations/clip-captions", "ViT-B/32") == \
        "/data/coco/annotations/ViT-B-32_clip_features"
    res = str(tmp_path / "res")
    clip_score.write_result(res, "coco", "/gen/a", 30.25)
    clip_score.write_result(res, "coco", "/gen/b", 31.5)
    assert open(os.path.join(res, "clip_score_coco.txt")).read() == "/gen/a 30.25\n/gen/b 31.5\n"


def test_clip_features_rejects_image_dirs(tmp_path):
    from pdm.utils.clip_utils import clip_features
    np.save(str(tmp_path / "a.npy"), np.zeros((2, 2, 3), np.uint8))
    with pytest.raises(ValueError, match="captions"):
        clip_features(str(tmp_path), clip_model="ViT-B/32")
