"""The HIP CLIP model of the CLIP score (-m gpu): the new kernels against torch on the device, and both towers against the
committed outputs of transformers.CLIPModel (tests/golden/clip_score_hf.npz, tools/make_clip_score_golden.py).
Tolerances: fp32 3e-4 of the output scale; bf16 per-row cosine >= 0.999 to the reference embedding."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_score_fixtures as fx

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "clip_score_hf.npz"))


def close(got, ref, tol, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_quick_gelu(dev, dn):
    from pdm import _pdmk as k
    x = (torch.randn(37, 1000, device=dev, generator=torch.Generator(dev).manual_seed(1)) * 4).to(DT[dn])
    y = torch.empty_like(x)
    k.quick_gelu_fwd(x, y)
    xf = x.float()
    close(y, xf * torch.sigmoid(1.702 * xf), 2e-6 if dn == "f32" else 1e-2, "quick_gelu")


@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_im2col_and_tokens(dev, dn):
    from pdm import _pdmk as k
    g = torch.Generator(dev).manual_seed(2)
    B, S, p, E = 3, 64, 16, 96
    G, K, ld = S // p, 3 * p * p, 3 * p * p + 32
    x = torch.randn(B, 3, S, S, device=dev, generator=g)
    cols = torch.full((B * G * G, ld), float("nan"), device=dev).to(DT[dn])
    k.patch_im2col(x, cols, B, S, p)
    ref = x.view(B, 3, G, p, G, p).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, K)
    close(cols[:, :K], ref, 0 if dn == "f32" else 1e-2, "im2col")
    assert (cols[:, K:].float() == 0).all()
    w = torch.randn(E, 3, p, p, device=dev, generator=g)
    conv = F.conv2d(x, w, stride=p).flatten(2).transpose(1, 2)                   # [B, G2, E]: the conv is the GEMM
    close(cols[:, :K].float() @ w.reshape(E, K).t(), conv.reshape(B * G * G, E), 1e-4 if dn == "f32" else 2e-2, "conv")
    patches = torch.randn(B * G * G, E + 32, device=dev, generator=g).to(DT[dn])
    cls = torch.randn(E, device=dev, generator=g).to(DT[dn])
    pos = torch.randn(G * G + 1, E + 64, device=dev, generator=g).to(DT[dn])
    out = torch.empty(B * (G * G + 1), E, device=dev, dtype=DT[dn])
    k.vit_tokens(patches, cls, pos, E + 64, out, B, G * G, E)
    emb = torch.cat([cls.float().expand(B, 1, E), patches[:, :E].float().view(B, G * G, E)], 1) + pos[:, :E].float()
    close(out.view(B, G * G + 1, E), emb, 1e-7 if dn == "f32" else 1e-2, "tokens")


@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_pooling_and_score_head(dev, dn):
    from pdm import _pdmk as k
    g = torch.Generator(dev).manual_seed(3)
    B, T, D = 5, 77, 96
    x = torch.randn(B * T, D + 32, device=dev, generator=g).to(DT[dn])
    ids = torch.from_numpy(fx.text_ids("tiny", n=B)).to(dev)
    ids[2, 40] = ids[2, 6]                                  # a second EOT: the first one is pooled
    out = torch.empty(B, D, device=dev, dtype=DT[dn])
    k.gather_rows(x, ids, T, out, B, D)
    first = torch.tensor([int((r == r.max()).nonzero()[0]) for r in ids.cpu()])
    assert torch.equal(out.cpu(), x.view(B, T, D + 32)[torch.arange(B), first, :D].cpu())
    k.gather_rows(x, None, T, out, B, D)
    assert torch.equal(out.cpu(), x.view(B, T, D + 32)[:, 0, :D].cpu())
    a = torch.randn(B, D + 8, device=dev, generator=g)
    b = torch.randn(B, D, device=dev, generator=g)
    an, bn = torch.empty(B, D, device=dev), torch.empty(B, D, device=dev)
    acc = torch.full((1,), 0.25, device=dev, dtype=torch.float64)
    k.clip_score_head(a, b, an, bn, acc, B, D)
    ra, rb = F.normalize(a[:, :D].double(), dim=1), F.normalize(b.double(), dim=1)
    close(an, ra, 1e-6, "an")
    close(bn, rb, 1e-6, "bn")
    assert abs(acc.item() - 0.25 - (ra * rb).sum().item()) < 1e-5


def _model(tag, dn, dev, graph=True):
    from pdm.models.clip.clip_model import CLIPModel
    text, vision, proj = fx.CONFIGS[tag]
    m = CLIPModel.from_configs(text, vision, proj, device=dev, dtype=DT[dn], init=False)
    m.load_state_dict(fx.state_dict(tag))
    m.use_graph = graph
    return m


def _pixels(dev, arrays):
    from pdm.utils.clip_utils import pack_images, prep_images
    packed, desc = pack_images(arrays, 224)
    return prep_images(packed, desc, 224, dev)


def _check(got, ref, dn, what):
    if dn == "f32":
        close(got, ref, 3e-4, what)
    else:
        cos = F.cosine_similarity(got.float().cpu(), ref.float(), dim=1)
        assert cos.min().item() >= 0.999, f"{what}: per-row cosine {cos.tolist()}"


@pytest.mark.parametrize("dn", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["tiny", "b32"])
def test_towers_match_transformers(dev, dn, tag):
    m = _model(tag, dn, dev)
    n_img, n_txt = GOLD[f"{tag}_img"].shape[0], GOLD[f"{tag}_txt"].shape[0]
    img = m.encode_image(_pixels(dev, fx.model_images(n_img)))
    assert img.shape == (n_img, fx.CONFIGS[tag][2]) and img.dtype == torch.float32
    _check(img, torch.from_numpy(GOLD[f"{tag}_img"]), dn, f"image[{tag}]")
    txt = m.encode_text(torch.from_numpy(fx.text_ids(tag, n=n_txt)))
    _check(txt, torch.from_numpy(GOLD[f"{tag}_txt"]), dn, f"text[{tag}]")
    if dn == "f32":                                          # graph replay == eager, twice over
        m.use_graph = False
        ids = torch.from_numpy(fx.text_ids(tag, n=n_txt))
        assert torch.equal(m.encode_text(ids), txt) and torch.equal(m.encode_text(ids), txt)


def test_weight_formats_identical(dev, tmp_path):
    """A transformers directory, a pickled OpenAI state dict and a TorchScript-free OpenAI .pt give the same outputs."""
    from pdm.models.clip.clip_model import CLIPModel
    from test_clip_score import hf_to_openai
    d = fx.write_hf_dir(str(tmp_path), "tiny")
    pt = tmp_path / "ViT-tiny.pt"
    torch.save(hf_to_openai(fx.state_dict("tiny")), str(pt))
    a = CLIPModel.from_pretrained(d, device=dev)
    b = CLIPModel.from_pretrained(str(pt), device=dev)
    px = _pixels(dev, fx.model_images(2))
    ids = torch.from_numpy(fx.text_ids("tiny", n=3))
    assert torch.equal(a.encode_image(px), b.encode_image(px))
    assert torch.equal(a.encode_text(ids), b.encode_text(ids))
    assert float(a.logit_scale) == float(b.logit_scale)
