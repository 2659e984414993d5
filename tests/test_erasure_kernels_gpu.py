"""pdmk_cosine_pairs (csrc/clip.hip) and pdmk_image_to_u8_ex (csrc/sampler.hip), -m gpu: the artist-erasure score's head
against torch.nn.functional.cosine_similarity in fp64, and the rounding uint8 conversion against numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5          # absolute, on a cosine: the bound of the unit-norm check of tests/test_clip_score_gpu.py
MARGIN = 1e-4       # fp64 |cos_b - cos_a| above which the fp32 flag must equal the fp64 comparison (10 x TOL)
ZERO_ROW, EQUAL_ROW = 0, 1


def _inputs(B, D, pad, seed):
    """t, a, b as [B, D] views of wider buffers (row strides D + pad, D + pad + 3, D + pad + 8; the padding holds large
    values the kernel must not read).  b = a + noise, so the two cosines differ by ~0.1 on most rows.  Row 0 of `a` is
    zero; row 1 has a == b (B > 1)."""
    g = torch.Generator().manual_seed(seed)
    bufs = [torch.full((B, D + pad + extra), 1e6) for extra in (0, 3, 8)]
    t, a, b = (buf[:, :D] for buf in bufs)
    t.copy_(torch.randn(B, D, generator=g))
    a.copy_(torch.randn(B, D, generator=g) + 0.3 * t)
    b.copy_(a + 0.4 * torch.randn(B, D, generator=g))
    a[ZERO_ROW] = 0
    if B > 1:
        b[EQUAL_ROW] = a[EQUAL_ROW]
    return bufs, (t, a, b)


def _run(k, dev, bufs, D, rows=None):
    t, a, b = (buf.to(dev)[:, :D] for buf in bufs)
    if rows is not None:
        t, a, b = t[rows], a[rows], b[rows]
    B = t.shape[0]
    sa = torch.full((B,), 7.0, device=dev)
    sb = torch.full((B,), 7.0, device=dev)
    lt = torch.full((B,), 7, device=dev, dtype=torch.int32)
    k.cosine_pairs(t, a, b, sa, sb, lt)
    return sa.cpu(), sb.cpu(), lt.cpu()


@pytest.mark.parametrize("D", [64, 200, 512])
@pytest.mark.parametrize("B", [1, 7, 300])
def test_cosine_pairs_against_fp64(dev, B, D):
    from pdm import _pdmk as k
    bufs, (t, a, b) = _inputs(B, D, pad=5, seed=B * 1000 + D)
    assert all(buf.stride(0) > D for buf in bufs)
    sa, sb, lt = _run(k, dev, bufs, D)
    ra = torch.nn.functional.cosine_similarity(t.double(), a.double(), dim=1)
    rb = torch.nn.functional.cosine_similarity(t.double(), b.double(), dim=1)
    assert torch.isfinite(sa).all() and torch.isfinite(sb).all()
    ea, eb = (sa.double() - ra).abs().max().item(), (sb.double() - rb).abs().max().item()
    print(f"B {B} D {D}: max |err| {ea:.2e} {eb:.2e}")
    assert ea <= TOL and eb <= TOL
    assert sa[ZERO_ROW].item() == 0.0 and ra[ZERO_ROW].item() == 0.0                 # clamped norm: 0, not NaN
    assert set(lt.tolist()) <= {0, 1}
    assert torch.equal(lt, (sb < sa).to(torch.int32))                                 # compared on the stored fp32 values
    if B > 1:
        assert lt[EQUAL_ROW].item() == 0 and sa[EQUAL_ROW].item() == sb[EQUAL_ROW].item()
    clear = (rb - ra).abs() > MARGIN
    assert (~clear).sum().item() <= max(1, B // 10), (~clear).sum().item()            # at most one row in ten is a near tie
    assert torch.equal(lt[clear], (rb < ra).to(torch.int32)[clear])
    if B >= 7:
        assert 0 < lt.sum().item() < B                                                # both outcomes occur


def test_cosine_pairs_does_not_depend_on_the_batch_split(dev):
    from pdm import _pdmk as k
    B, D = 300, 512
    bufs, _ = _inputs(B, D, pad=5, seed=9)
    whole = _run(k, dev, bufs, D)
    parts = [_run(k, dev, bufs, D, rows=slice(s, min(s + 64, B))) for s in range(0, B, 64)]
    for j in range(3):
        assert torch.equal(torch.cat([p[j] for p in parts]), whole[j])
    # compare bit patterns as well: -0.0 == 0.0 would pass torch.equal
    assert torch.equal(torch.cat([p[0] for p in parts]).view(torch.int32), whole[0].view(torch.int32))
    assert torch.equal(torch.cat([p[1] for p in parts]).view(torch.int32), whole[1].view(torch.int32))


def test_cosine_pairs_rejects_bad_arguments(dev):
    from pdm import _pdmk as k
    t = torch.zeros(4, 64, device=dev)
    s, lt = torch.zeros(4, device=dev), torch.zeros(4, device=dev, dtype=torch.int32)
    with pytest.raises(k.PdmkError):
        k.cosine_pairs(t, t[:, :32], t, s, s.clone(), lt)
    with pytest.raises(k.PdmkError):
        k.cosine_pairs(t, t, t, s, s.clone(), lt.float())
    with pytest.raises(k.PdmkError):
        k.cosine_pairs(t, t, t, s[:3], s.clone(), lt)


def _halves():
    """fp32 inputs x whose chain fp32(fp32(x / 2 + 0.5) * 255) lands exactly on m + 0.5: a host search around the exact
    preimages (m + 0.5) / 255 * 2 - 1."""
    found = []
    for m in range(255):
        c = np.float32((m + 0.5) / 255 * 2 - 1)
        x = c
        for _ in range(8):                                   # 8 fp32 neighbours below and above
            x = np.nextafter(x, np.float32(-2))
        for _ in range(17):
            v = np.float32(np.float32(x / np.float32(2) + np.float32(0.5)) * np.float32(255))
            if v == np.float32(m + 0.5):
                found.append(x)
            x = np.nextafter(x, np.float32(2))
    return np.asarray(found, np.float32)


def _u8_input():
    B, C, H, W = 2, 3, 16, 16
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, H, W, generator=g) * 1.2          # spans below -1 to above 1
    flat = x.view(-1)
    halves = torch.from_numpy(_halves())
    assert halves.numel() >= 16, halves.numel()              # there are inputs that land exactly on .5 ...
    special = torch.cat([torch.tensor([float("nan"), 1.0, -1.0, 1.0000001, -1.0000001, 1.5, -1.5, 0.0, -0.0, float("inf"),
                                       -float("inf")]), halves[:700]])
    assert special.numel() < flat.numel() // 2
    flat[:special.numel()] = special
    fin = flat[torch.isfinite(flat)]
    assert fin.min() < -1 and fin.max() > 1 and torch.isnan(flat).any()
    return x, halves


def test_image_to_u8_ex_rounds_like_numpy(dev):
    from pdm import _pdmk as k
    x, halves = _u8_input()
    B, C, H, W = x.shape
    img = (x / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy()              # fp32, on the host: exact operations
    img = np.where(np.isnan(img), np.float32(0), img)                         # the kernel's NaN -> 0 (a NaN has no uint8)
    prod = img * np.float32(255)
    n_half = int((prod - np.floor(prod) == 0.5).sum())
    assert n_half >= 16, n_half                                               # ... and they reach the rounding step
    both = prod[prod - np.floor(prod) == 0.5]
    assert (np.floor(both) % 2 == 0).any() and (np.floor(both) % 2 == 1).any()  # ties below even and below odd values
    want = prod.round().astype(np.uint8)
    got = torch.empty(B, H, W, C, device=dev, dtype=torch.uint8)
    k.image_to_u8_ex(x.to(dev).contiguous(), got, 1)
    assert np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(want, prod.astype(np.uint8))                    # rounding differs from truncation here


def test_image_to_u8_ex_rounding_0_is_image_to_u8(dev):
    from pdm import _pdmk as k
    x, _ = _u8_input()
    B, C, H, W = x.shape
    xd = x.to(dev).contiguous()
    a = torch.empty(B, H, W, C, device=dev, dtype=torch.uint8)
    b = torch.full((B, H, W, C), 9, device=dev, dtype=torch.uint8)
    k.image_to_u8(xd, a)
    k.image_to_u8_ex(xd, b, 0)
    assert torch.equal(a, b)
    with pytest.raises(k.PdmkError):
        k.image_to_u8_ex(xd, b, 2)


def test_pipeline_u8_round_output(dev):
    """output_type="u8_round" is numpy's rounding of the pipeline's float image, "u8" stays its truncation."""
    from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
    from pdm.pipelines.pruning_pipelines import StableDiffusionPruningPipeline
    cfg = UNetConfig.tiny()
    av = arch_vector_for_budget(cfg, 0.6, hw=16)[0]
    unet = UNet2DConditionModelPruned(cfg, av, dev, torch.float32, train=False, seed=0)
    vae = AutoencoderKL(VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1), dev, torch.float32, seed=1)
    pipe = StableDiffusionPruningPipeline(vae, None, unet)
    g = torch.Generator(device=dev).manual_seed(3)
    emb = torch.randn(1, 13, cfg.cross_attention_dim, device=dev, generator=g)
    neg = torch.randn(1, 13, cfg.cross_attention_dim, device=dev, generator=g)
    lat = torch.randn(1, 4, 16, 16, device=dev, generator=g)
    out = {t: pipe(prompt_embeds=emb, negative_prompt_embeds=neg, latents=lat, num_inference_steps=2, output_type=t,
                   graph=False).images for t in ("np", "u8", "u8_round")}
    assert out["u8_round"].dtype == np.uint8 and out["u8_round"].shape == out["u8"].shape
    assert np.array_equal(out["u8"], (out["np"] * 255).astype(np.uint8))
    assert np.array_equal(out["u8_round"], (out["np"] * 255).round().astype(np.uint8))
    assert not np.array_equal(out["u8"], out["u8_round"])
