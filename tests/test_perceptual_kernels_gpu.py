"""The three kernels of csrc/perceptual.hip, one by one against torch on the CPU.  pdmk_relu_pool is bit-equal; the two metric
heads are measured with the project's yardstick (tests/test_fid_gpu.py): error against the float64 restatement, relative to
the output, at most 8 x that of the same restatement in float32, floor 8 fp32 ulps - on inputs for which float32 itself is
within 1e-5 of float64 (asserted).  The Gram inputs of a pair differ in per-channel scale and offset: two maps of plain noise
have nearly the same Gram matrix at large HW, G_0 - G_1 cancels and float32 stops being a yardstick."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perceptual_fixtures as fx  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = -123.25


def _k():
    from pdm import _pdmk
    return _pdmk


def _sliced(x, off, extra, fill=7.0):
    """x [rows, C] as columns [off, off + C) of a CPU buffer with rows of C + extra."""
    buf = torch.full((x.shape[0], x.shape[1] + extra), fill)
    buf[:, off:off + x.shape[1]] = x
    return buf


# ---------------------------------------------------------------------------------------------------- relu_pool
@pytest.mark.parametrize("pool", [0, 2])
@pytest.mark.parametrize("H,W", [(37, 41), (2, 2), (1, 1)])
@pytest.mark.parametrize("C", [64, 200])
def test_relu_pool_bit_equal(dev, pool, H, W, C):
    k = _k()
    B = 2
    g = torch.Generator().manual_seed(H * 100 + C + pool)
    x = torch.randn(B, H, W, C, generator=g)
    xb = _sliced(x.reshape(-1, C), 4, 12).to(dev)
    xs = xb[:, 4:4 + C]
    if pool == 2 and min(H, W) < 2:
        y = torch.zeros(B, C, device=dev)
        assert k._lib.pdmk_relu_pool(xs.data_ptr(), xb.stride(0), y.data_ptr(), C, B, H, W, C, 2, None) == -1
        return
    xn = x.permute(0, 3, 1, 2)
    ref = F.relu(xn) if pool == 0 else F.max_pool2d(F.relu(xn), 2, 2)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    Ho, Wo = ref.shape[1:3]
    assert (Ho, Wo) == ((H, W) if pool == 0 else (H // 2, W // 2))
    yb = torch.full((B * Ho * Wo, C + 20), CANARY, device=dev)
    k.relu_pool(xs, xb.stride(0), yb[:, 8:8 + C], yb.stride(0), B, H, W, C, pool)
    yb = yb.cpu()
    assert torch.equal(yb[:, 8:8 + C].reshape(ref.shape), ref)
    assert bool((yb[:, :8] == CANARY).all()) and bool((yb[:, 8 + C:] == CANARY).all()), "columns outside the slice were written"
    assert torch.equal(xb.cpu()[:, :4], torch.full((B * H * W, 4), 7.0))


def test_relu_in_place_and_nan(dev):
    k = _k()
    x = torch.tensor([[-1.0, float("nan"), 2.0, -0.0]]).repeat(6, 1)
    xd = x.to(dev)
    k.relu_pool(xd, 4, xd, 4, 1, 2, 3, 4, 0)
    got = xd.cpu()
    assert torch.equal(got[:, [0, 2, 3]], torch.tensor([[0.0, 2.0, 0.0]]).repeat(6, 1)) and bool(got[:, 1].isnan().all())


# ---------------------------------------------------------------------------------------------------- lpips_layer
def _lpips_inputs(B, HW, C, seed):
    """Post-ReLU-like maps; some pixels all-zero in one map, some in both."""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.randn(B, HW, C, generator=g).clamp_min(0)
    f1 = (f0 * 0.5 + torch.randn(B, HW, C, generator=g)).clamp_min(0)
    if HW >= 9:
        f0[:, 1] = 0
        f1[:, 3] = 0
        f0[:, 5] = 0
        f1[:, 5] = 0
    w = torch.rand(C, generator=g)
    return f0, f1, w


def _lpips_ref(f0, f1, w, dtype):
    f0, f1, w = f0.to(dtype), f1.to(dtype), w.to(dtype)
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(-1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(-1, keepdim=True)) + 1e-10)
    return (((n0 - n1) ** 2) * w).sum(-1).mean(-1).double().numpy()


def _check(ref, cpu32, got, what):
    bad = fx.yardstick(ref, cpu32, got, what)
    assert not bad, bad


@pytest.mark.parametrize("HW,C", [(225, 64), (49, 192), (9, 384), (1, 256)])
def test_lpips_layer(dev, HW, C):
    k = _k()
    B = 3
    f0, f1, w = _lpips_inputs(B, HW, C, HW + C)
    ref, cpu32 = _lpips_ref(f0, f1, w, torch.float64), _lpips_ref(f0, f1, w, torch.float32)
    assert np.isfinite(ref).all() and (ref > 0).all()
    d0, d1, wd = f0.reshape(-1, C).to(dev), f1.reshape(-1, C).to(dev), w.to(dev)
    out = torch.zeros(B, device=dev, dtype=torch.float64)
    k.lpips_layer(d0, d1, C, wd, out, B, HW, C)
    once = out.cpu().numpy().copy()
    _check(ref, cpu32, once, f"lpips_layer HW={HW} C={C}")
    k.lpips_layer(d0, d1, C, wd, out, B, HW, C)               # accumulates
    assert np.array_equal(out.cpu().numpy(), once + once)
    same = torch.zeros(B, device=dev, dtype=torch.float64)
    k.lpips_layer(d0, d0.clone(), C, wd, same, B, HW, C)
    assert np.array_equal(same.cpu().numpy(), np.zeros(B)), "an identical pair must give exactly 0.0"


def test_lpips_layer_unaligned_slice(dev):
    """Column offset 3 in rows of C + 5 (odd stride, unaligned base) and C = 70 (not a multiple of 4): the element path."""
    k = _k()
    B, HW, C = 3, 49, 70
    f0, f1, w = _lpips_inputs(B, HW, C, 99)
    ref, cpu32 = _lpips_ref(f0, f1, w, torch.float64), _lpips_ref(f0, f1, w, torch.float32)
    b0, b1 = _sliced(f0.reshape(-1, C), 3, 5).to(dev), _sliced(f1.reshape(-1, C), 3, 5).to(dev)
    out = torch.zeros(B, device=dev, dtype=torch.float64)
    k.lpips_layer(b0[:, 3:3 + C], b1[:, 3:3 + C], C + 5, w.to(dev), out, B, HW, C)
    _check(ref, cpu32, out.cpu().numpy(), "lpips_layer unaligned")


# ---------------------------------------------------------------------------------------------------- gram_pair
def _gram_inputs(B, HW, C, seed):
    g = torch.Generator().manual_seed(seed)
    maps = []
    for _ in range(2):
        scale, shift = torch.rand(B, 1, C, generator=g) + 0.5, torch.randn(B, 1, C, generator=g) * 0.5
        maps.append(torch.randn(B, HW, C, generator=g) * scale + shift)
    return maps


def _gram_ref(f0, f1, dtype):
    f0, f1 = f0.to(dtype), f1.to(dtype)
    B, HW, C = f0.shape
    g0 = torch.bmm(f0.transpose(1, 2), f0) / (C * HW)
    g1 = torch.bmm(f1.transpose(1, 2), f1) / (C * HW)
    return ((g0 - g1) ** 2).mean((1, 2)).double().numpy(), ((f0 - f1) ** 2).mean((1, 2)).double().numpy()


GRAM_CASES = [(5, 64), (37 * 41, 128), (96 * 96, 64), (24 * 24, 256)]     # less than one chunk, a ragged tail, many splits, 10 tiles


@pytest.mark.parametrize("HW,C", GRAM_CASES)
def test_gram_pair(dev, HW, C):
    k = _k()
    B = 2
    f0, f1 = _gram_inputs(B, HW, C, HW + C)
    (s64, c64), (s32, c32) = _gram_ref(f0, f1, torch.float64), _gram_ref(f0, f1, torch.float32)
    assert abs(s64[0] - s64[1]) > 1e-3 * s64[0], "fixture: the two images give the same loss"
    d0, d1 = f0.reshape(-1, C).to(dev), f1.reshape(-1, C).to(dev)
    n = k.gram_workspace_elems(B, HW, C)
    ws = torch.empty(n, device=dev)

    def run(content=True, a=d0, b=d1, ws=ws):
        style = torch.zeros(B, device=dev, dtype=torch.float64)
        cont = torch.zeros(B, device=dev, dtype=torch.float64) if content else None
        k.gram_pair(a, b, C, B, HW, C, ws, style, cont)
        return style.cpu().numpy(), (cont.cpu().numpy() if content else None)

    s1, c1 = run()
    _check(s64, s32, s1, f"gram style HW={HW} C={C}")
    _check(c64, c32, c1, f"gram content HW={HW} C={C}")
    s2, c2 = run()
    assert np.array_equal(s1, s2) and np.array_equal(c1, c2), "two launches must give the same bits"
    s3, c3 = run(content=False)
    assert c3 is None and np.array_equal(s3, s1)
    s4, c4 = run(b=d0.clone())
    assert np.array_equal(s4, np.zeros(B)) and np.array_equal(c4, np.zeros(B)), "an identical pair must give exactly 0.0"
    with pytest.raises(k.PdmkError):
        run(ws=ws[:n - 1])
    style = torch.zeros(B, device=dev, dtype=torch.float64)      # accumulates into the outputs
    k.gram_pair(d0, d1, C, B, HW, C, ws, style, None)
    k.gram_pair(d0, d1, C, B, HW, C, ws, style, None)
    assert np.array_equal(style.cpu().numpy(), s1 + s1)


def test_gram_pair_sliced_unaligned(dev):
    """C = 70 at column offset 3 of rows of 75: the element loads, two column tiles with a ragged second one."""
    k = _k()
    B, HW, C = 2, 300, 70
    f0, f1 = _gram_inputs(B, HW, C, 7)
    (s64, c64), (s32, c32) = _gram_ref(f0, f1, torch.float64), _gram_ref(f0, f1, torch.float32)
    b0, b1 = _sliced(f0.reshape(-1, C), 3, 5, 1e3).to(dev), _sliced(f1.reshape(-1, C), 3, 5, -1e3).to(dev)
    ws = torch.empty(k.gram_workspace_elems(B, HW, C), device=dev)
    style = torch.zeros(B, device=dev, dtype=torch.float64)
    cont = torch.zeros(B, device=dev, dtype=torch.float64)
    k.gram_pair(b0[:, 3:3 + C], b1[:, 3:3 + C], C + 5, B, HW, C, ws, style, cont)
    _check(s64, s32, style.cpu().numpy(), "gram style sliced")
    _check(c64, c32, cont.cpu().numpy(), "gram content sliced")


# ---------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments(dev):
    k = _k()
    lib = k._lib
    x = torch.zeros(64, 8, device=dev)
    y = torch.zeros(64, 8, device=dev)
    w = torch.zeros(8, device=dev)
    o = torch.zeros(4, device=dev, dtype=torch.float64)
    ws = torch.zeros(int(k.gram_workspace_elems(1, 64, 8)), device=dev)
    px, py, pw, po, pws = (t.data_ptr() for t in (x, y, w, o, ws))
    # relu_pool: null, stride < row, size < 1, unknown pool, misaligned
    assert lib.pdmk_relu_pool(None, 8, py, 8, 1, 8, 8, 8, 0, None) == -1
    assert lib.pdmk_relu_pool(px, 4, py, 8, 1, 8, 8, 8, 0, None) == -1
    assert lib.pdmk_relu_pool(px, 8, py, 8, 0, 8, 8, 8, 0, None) == -1
    assert lib.pdmk_relu_pool(px, 8, py, 8, 1, 8, 8, 8, 3, None) == -1
    assert lib.pdmk_relu_pool(px + 2, 8, py, 8, 1, 4, 4, 8, 0, None) == -1
    # lpips_layer
    assert lib.pdmk_lpips_layer(px, None, 8, pw, po, 1, 64, 8, None) == -1
    assert lib.pdmk_lpips_layer(px, py, 4, pw, po, 1, 64, 8, None) == -1
    assert lib.pdmk_lpips_layer(px, py, 8, pw, po, 1, 0, 8, None) == -1
    assert lib.pdmk_lpips_layer(px, py, 8, pw, po + 4, 1, 64, 8, None) == -1
    # gram_pair
    assert lib.pdmk_gram_pair(px, py, 8, 1, 64, 8, None, ws.numel(), po, None, None) == -1
    assert lib.pdmk_gram_pair(px, py, 4, 1, 64, 8, pws, ws.numel(), po, None, None) == -1
    assert lib.pdmk_gram_pair(px, py, 8, 1, 64, 0, pws, ws.numel(), po, None, None) == -1
    assert lib.pdmk_gram_pair(px, py, 8, 1, 64, 8, pws + 4, ws.numel(), po, None, None) == -1
    assert lib.pdmk_gram_pair(px, py, 8, 1, 64, 8, pws, ws.numel(), po, po + 4, None) == -1
    assert lib.pdmk_gram_workspace_elems(0, 64, 8) == -1 and lib.pdmk_gram_workspace_elems(1, 64, 4096) == -1
    with pytest.raises(k.PdmkError):
        k.lpips_layer(x, y, 8, w, o, 2, 64, 8)                 # B larger than the buffers
    with pytest.raises(k.PdmkError):
        k.relu_pool(x, 8, y, 8, 2, 8, 8, 8, 0)
    torch.cuda.synchronize()
    assert float(o.abs().sum()) == 0.0 and float(y.abs().sum()) == 0.0, "a refused call wrote"
