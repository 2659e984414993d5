"""The two kernels of the object-erasure classifier on the GPU: pdmk_conv2d_fwd_res (the implicit-GEMM conv with a residual
operand in the epilogue) against F.conv2d + res on the CPU, and pdmk_softmax_topk against a float64 softmax and this project's
tie rule.  Yardstick as tests/test_fid_gpu.py: error against float64 relative to the output's scale, at most 8 x the float32
restatement's own error, floor 8 fp32 ulps."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_fixtures as fx  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = -123.25


def _k():
    from pdm import _pdmk
    return _pdmk


# ---------------------------------------------------------------------------------------------------- conv + residual
# (Ci, Co, kh, kw, stride, pad, H, W, B).  Tiles are 64 rows x 64 columns (128 rows in the large-M forms).
CONV_CASES = {
    "1x1_64to256_9x12_b1": (64, 256, 1, 1, 1, 0, 9, 12, 1),          # M = 108
    "1x1_64to256_9x12_b3": (64, 256, 1, 1, 1, 0, 9, 12, 3),          # M = 324
    "1x1_s2_9x11_b1": (64, 128, 1, 1, 2, 0, 9, 11, 1),               # odd map, stride 2: 5 x 6
    "1x1_s2_9x11_b3": (64, 128, 1, 1, 2, 0, 9, 11, 3),
    "3x3_p1_5x6_b1": (64, 64, 3, 3, 1, 1, 5, 6, 1),
    "3x3_p1_5x6_b3": (64, 64, 3, 3, 1, 1, 5, 6, 3),
    "m63": (64, 64, 1, 1, 1, 0, 7, 9, 1),
    "m65": (64, 64, 1, 1, 1, 0, 5, 13, 1),
    "m127": (64, 64, 1, 1, 1, 0, 1, 127, 1),
    "m129": (64, 64, 1, 1, 1, 0, 3, 43, 1),
    "co70_ci3_elementwise": (3, 70, 3, 3, 1, 1, 9, 12, 1),           # column tail, element gathers
    "large_m_wm2": (64, 256, 1, 1, 1, 0, 127, 129, 1),               # M = 16383: 128 x 4 workgroups of 128 rows, M tail 127
    "large_m_wm2_ci3": (3, 70, 1, 1, 1, 0, 181, 181, 1),             # M = 32761: the element-gather form with 128 rows
}
LARGE = {"large_m_wm2", "large_m_wm2_ci3"}


def _conv_setup(case, seed=0):
    Ci, Co, kh, kw, s, p, H, W, B = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Ci, generator=g).abs()
    w = torch.randn(Co, Ci, kh, kw, generator=g) * (2.0 / (Ci * kh * kw)) ** 0.5
    b = torch.randn(Co, generator=g) * 0.2
    Ho, Wo = (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1
    res = torch.randn(B, Ho, Wo, Co, generator=g)
    return x, w, b, res, Ho, Wo


def _reference(x, w, b, res, s, p, relu, dtype):
    y = F.conv2d(x.permute(0, 3, 1, 2).to(dtype), w.to(dtype), b.to(dtype), s, p) + res.permute(0, 3, 1, 2).to(dtype)
    return (F.relu(y) if relu else y).double()


def _launch(dev, case, x, w, b, res, Ho, Wo, relu, ldr_extra=8, ldc_extra=40, o0=16, r0=4):
    """Output columns [o0, o0 + Co) of rows of ldc, residual columns [r0, r0 + Co) of rows of ldr; returns the whole buffers."""
    k = _k()
    Ci, Co, kh, kw, s, p, H, W, B = case
    M = B * Ho * Wo
    yb = torch.full((M, Co + ldc_extra), CANARY, device=dev)
    rb = torch.full((M, Co + ldr_extra), 9.5)
    rb[:, r0:r0 + Co] = res.reshape(M, Co)
    rb = rb.to(dev)
    wk = w.permute(0, 2, 3, 1).reshape(Co, -1).contiguous().to(dev)
    xd = x.reshape(-1, Ci).to(dev)
    k.conv2d_fwd_res(xd, Ci, wk, b.to(dev), rb[:, r0:r0 + Co], Co + ldr_extra, yb[:, o0:o0 + Co], Co + ldc_extra, B, H, W, Ci, Co,
                     kh, kw, s, p, p, relu=relu)
    return yb.cpu(), rb.cpu()


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv2d_fwd_res(dev, name, relu):
    """Against F.conv2d + bias + res (+ ReLU); res and y are column slices of wider buffers (ldr > Co, ldc > Co) and every
    column outside the output slice keeps its canary; the residual buffer is not written."""
    case = CONV_CASES[name]
    Ci, Co, kh, kw, s, p, H, W, B = case
    x, w, b, res, Ho, Wo = _conv_setup(case)
    M = B * Ho * Wo
    if name in LARGE:
        assert -(-M // 128) * -(-Co // 64) >= 512 and M % 128, "fixture: not a 128-row-tile case with an M tail"
    else:
        assert -(-M // 128) * -(-Co // 64) < 512, "fixture: not a 64-row-tile case"
    ref = _reference(x, w, b, res, s, p, relu, torch.float64)
    cpu32 = _reference(x, w, b, res, s, p, relu, torch.float32)
    scale = ref.abs().max().item()
    yard = max(8 * (cpu32 - ref).abs().max().item(), 8 * fx.ulp32(scale))
    yb, rb = _launch(dev, case, x, w, b, res, Ho, Wo, relu)
    got = yb[:, 16:16 + Co].reshape(B, Ho, Wo, Co).permute(0, 3, 1, 2).double()
    err = (got - ref).abs().max().item()
    print(f"conv_res {name} relu={relu}: M={M} err/max {err / scale:.3e}, yardstick/max {yard / scale:.3e}")
    assert bool((torch.cat([yb[:, :16], yb[:, 16 + Co:]], 1) == CANARY).all()), "columns outside the output slice were written"
    assert torch.equal(rb[:, 4:4 + Co], res.reshape(M, Co)) and bool((rb[:, :4] == 9.5).all()) and bool((rb[:, 4 + Co:] == 9.5).all())
    assert err <= yard, (err, yard)
    if not relu:
        assert (got < 0).any(), "fixture: the linear case has no negative output"


@pytest.mark.parametrize("name", ["1x1_64to256_9x12_b3", "3x3_p1_5x6_b3", "m129", "co70_ci3_elementwise", "large_m_wm2"])
def test_conv2d_fwd_res_in_place(dev, name):
    """res == y (same pointer, ldr == ldc): the result over the residual's own buffer equals the out-of-place one bit for bit."""
    k = _k()
    case = CONV_CASES[name]
    Ci, Co, kh, kw, s, p, H, W, B = case
    x, w, b, res, Ho, Wo = _conv_setup(case, seed=3)
    M = B * Ho * Wo
    wk = w.permute(0, 2, 3, 1).reshape(Co, -1).contiguous().to(dev)
    xd, bd = x.reshape(-1, Ci).to(dev), b.to(dev)
    out = torch.full((M, Co), CANARY, device=dev)
    k.conv2d_fwd_res(xd, Ci, wk, bd, res.reshape(M, Co).to(dev), Co, out, Co, B, H, W, Ci, Co, kh, kw, s, p, p, relu=True)
    buf = torch.full((M, Co + 8), CANARY, device=dev)           # in place inside a wider buffer: ldr == ldc == Co + 8
    buf[:, :Co] = res.reshape(M, Co).to(dev)
    k.conv2d_fwd_res(xd, Ci, wk, bd, buf[:, :Co], Co + 8, buf[:, :Co], Co + 8, B, H, W, Ci, Co, kh, kw, s, p, p, relu=True)
    assert torch.equal(buf[:, :Co].contiguous().view(torch.int32), out.view(torch.int32))
    assert bool((buf[:, Co:] == CANARY).all())


@pytest.mark.parametrize("name", ["1x1_64to256_9x12_b3", "3x3_p1_5x6_b1", "co70_ci3_elementwise", "large_m_wm2", "large_m_wm2_ci3"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_conv2d_fwd_res_null_is_conv2d_fwd(dev, name, relu):
    k = _k()
    case = CONV_CASES[name]
    Ci, Co, kh, kw, s, p, H, W, B = case
    x, w, b, res, Ho, Wo = _conv_setup(case, seed=4)
    M = B * Ho * Wo
    wk = w.permute(0, 2, 3, 1).reshape(Co, -1).contiguous().to(dev)
    xd, bd = x.reshape(-1, Ci).to(dev), b.to(dev)
    a = torch.full((M, Co), CANARY, device=dev)
    c = torch.full((M, Co), CANARY, device=dev)
    k.conv2d_fwd(xd, Ci, wk, bd, a, Co, B, H, W, Ci, Co, kh, kw, s, p, p, relu=relu)
    k.conv2d_fwd_res(xd, Ci, wk, bd, None, 0, c, Co, B, H, W, Ci, Co, kh, kw, s, p, p, relu=relu)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, b, s, p)
    ref = (F.relu(ref) if relu else ref).permute(0, 2, 3, 1).reshape(M, Co)
    assert torch.allclose(a.cpu(), ref, rtol=1e-4, atol=1e-4)


def test_conv2d_fwd_res_bad_arguments(dev):
    k = _k()
    x = torch.zeros(64, 8, device=dev)
    w = torch.zeros(8, 8, device=dev)
    y = torch.zeros(64, 8, device=dev)
    r = torch.zeros(64 * 8 + 4, device=dev)
    args = (1, 8, 8, 8, 8, 1, 1, 1, 0, 0)
    with pytest.raises(k.PdmkError):
        k.conv2d_fwd_res(x, 8, w, None, r, 4, y, 8, *args)                          # ldr < Co
    with pytest.raises(k.PdmkError):
        k.conv2d_fwd_res(x, 8, w, None, torch.zeros(32 * 8, device=dev), 8, y, 8, *args)   # res shorter than the output
    with pytest.raises(k.PdmkError):
        k.conv2d_fwd_res(x, 4, w, None, r, 8, y, 8, *args)                          # what conv2d_fwd rejects: lda < Ci
    with pytest.raises(k.PdmkError):
        k.conv2d_fwd_res(x, 8, w, None, r, 8, y, 4, *args)                          # ldc < Co
    # the library's own checks (nothing is launched on -1)
    st = torch.cuda.current_stream().cuda_stream

    def raw(res_ptr, ldr, lda=8):
        return k._lib.pdmk_conv2d_fwd_res(x.data_ptr(), lda, w.data_ptr(), None, res_ptr, ldr, y.data_ptr(), 8, *args, 1, st)

    assert raw(r.data_ptr(), 7) == -1                                                # ldr < Co
    assert raw(r.data_ptr() + 2, 8) == -1                                            # misaligned res
    assert raw(r.data_ptr(), 8, lda=4) == -1
    assert raw(None, 0) == 0 and raw(r.data_ptr(), 8) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- softmax + top-k
def _ladder_logits(B, N, seed):
    """Rows whose sorted values step down by 2 % of probability (0.02 in the logit), permuted, shifted and scaled per row: the
    gap condition holds by construction and is still asserted."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(B):
        z = -0.02 * torch.arange(N, dtype=torch.float64)
        z = z[torch.randperm(N, generator=g)] * (0.5 + 1.5 * torch.rand((), generator=g).item()) + torch.randn((), generator=g).item() * 3
        rows.append(z.to(torch.float32))
    return torch.stack(rows)


# (B, N, k, ld)
TOPK_CASES = {
    "n1000_k5_b1": (1, 1000, 5, 1000),
    "n1000_k5_b300": (300, 1000, 5, 1000),
    "n10_k10": (3, 10, 10, 10),
    "n1_k1": (2, 1, 1, 1),
    "n1024_k16": (5, 1024, 16, 1024),
    "n1025_k5": (3, 1025, 5, 1025),
    "n5000_k16_ld5008": (2, 5000, 16, 5008),
    "n1000_k5_b300_ld1024": (300, 1000, 5, 1024),
}


def _run_topk(dev, z, k_, ld):
    B, N = z.shape
    buf = torch.full((B, ld), float("inf"))                 # an element read past N would win every round
    buf[:, :N] = z
    buf = buf.to(dev)
    p, i = _k().softmax_topk(buf[:, :N], k_)
    return p.cpu().numpy().astype(np.float64), i.cpu().numpy().astype(np.int64), buf


@pytest.mark.parametrize("name", sorted(TOPK_CASES))
def test_softmax_topk(dev, name):
    """Probabilities by the yardstick, indices exact (the fixture's gap condition makes the order unambiguous)."""
    B, N, k_, ld = TOPK_CASES[name]
    z = _ladder_logits(B, N, seed=len(name) + N)
    p64, i64, p32 = fx.check_gaps(z.numpy().astype(np.float64), z.numpy(), k_, f"topk {name}")
    got_p, got_i, _ = _run_topk(dev, z, k_, ld)
    assert got_p.shape == (B, k_) and got_i.shape == (B, k_)
    assert np.array_equal(got_i, i64), (got_i[:2], i64[:2])
    bad = fx.yardstick(p64, p32, got_p, f"topk {name} probs")
    assert not bad, bad
    assert (np.diff(got_p, axis=1) <= 0).all()


def test_softmax_topk_large_logits(dev):
    """Logits 1e4 apart: exp(x - max) underflows to exactly 0 for everything but the maximum, nothing overflows."""
    z = torch.zeros(3, 1000)
    z[0, :8] = torch.arange(8) * 1e4
    z[1] = torch.arange(1000) * -1e4
    z[2] = torch.arange(1000) * 1e4 - 5e6
    p, i, _ = _run_topk(dev, z, 4, 1000)
    assert np.array_equal(p, np.array([[1.0, 0, 0, 0]] * 3))
    assert np.array_equal(i, np.array([[7, 6, 5, 4], [0, 1, 2, 3], [999, 998, 997, 996]]))


@pytest.mark.parametrize("N", [1000, 5000], ids=["registers", "reread"])
def test_softmax_topk_ties_ascending(dev, N):
    """Equal logits come lower index first, within a lane's own elements (columns 64 apart) and across lanes; -0 ties +0."""
    z = torch.full((4, N), -1.0)
    z[1, [700, 63, 64, 5, 69]] = 2.0                        # 5 and 69 share a lane, 63 / 64 are neighbours in different lanes
    z[2, [900, 3]] = 3.0
    z[2, [10, 11, N - 1]] = 1.0
    z[3] = 0.0
    z[3, 1::2] = -0.0
    p, i, _ = _run_topk(dev, z, 5, N)
    assert np.array_equal(i, np.array([[0, 1, 2, 3, 4], [5, 63, 64, 69, 700], [3, 900, 10, 11, N - 1], [0, 1, 2, 3, 4]])), i
    p64, _ = fx.softmax_topk(z.numpy().astype(np.float64), 5)
    assert np.abs(p - p64).max() <= 8 * fx.ulp32(p64.max())
    assert np.array_equal(p[0], np.full(5, p[0, 0])) and np.array_equal(p[3], np.full(5, p[3, 0]))


@pytest.mark.parametrize("N", [1000, 5000], ids=["registers", "reread"])
def test_softmax_topk_nan_row(dev, N):
    """A NaN ranks above everything, lower index first among NaNs, and every probability of its row is NaN; the other rows
    are untouched by it."""
    z = _ladder_logits(3, N, seed=N)
    clean = z.clone()
    z[1, 900] = float("nan")
    z[1, 17] = float("nan")
    z[1, 18] = float("inf")
    p, i, _ = _run_topk(dev, z, 5, N)
    _, want = fx.softmax_topk(z.numpy().astype(np.float64), 5)
    assert list(want[1][:3]) == [17, 900, 18]
    assert np.array_equal(i, want), (i, want)
    assert np.isnan(p[1]).all() and np.isfinite(p[[0, 2]]).all()
    pc, ic, _ = _run_topk(dev, clean, 5, N)
    assert np.array_equal(p[[0, 2]], pc[[0, 2]]) and np.array_equal(i[[0, 2]], ic[[0, 2]])


def test_softmax_topk_same_bits_twice(dev):
    z = _ladder_logits(300, 1000, seed=9).to(dev)
    k = _k()
    p1, i1 = k.softmax_topk(z, 5)
    p2, i2 = k.softmax_topk(z, 5)
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)) and torch.equal(i1, i2)


def test_softmax_topk_bad_arguments(dev):
    k = _k()
    z = torch.zeros(4, 1000, device=dev)
    for bad_k in (0, 17):
        with pytest.raises(k.PdmkError):
            k.softmax_topk(z, bad_k)
    with pytest.raises(k.PdmkError):
        k.softmax_topk(z[:, :8], 9)                                                  # k > N
    with pytest.raises(k.PdmkError):
        k.softmax_topk(torch.zeros(1, 65537, device=dev), 1)                         # N > 65536
    with pytest.raises(k.PdmkError):
        k.softmax_topk(z.double(), 5)
    with pytest.raises(k.PdmkError):
        k.softmax_topk(z.t(), 5)                                                     # column stride != 1
    with pytest.raises(k.PdmkError):
        k.softmax_topk(z, 5, probs=torch.zeros(4, 4, device=dev))
    p = torch.zeros(4, 5, device=dev)
    i = torch.zeros(4, 5, device=dev, dtype=torch.int32)
    st = torch.cuda.current_stream().cuda_stream

    def raw(zp, ld, B, N, kk, pp, ip):
        return k._lib.pdmk_softmax_topk(zp, ld, B, N, kk, pp, ip, st)

    good = (z.data_ptr(), 1000, 4, 1000, 5, p.data_ptr(), i.data_ptr())
    assert raw(*good) == 0
    assert raw(z.data_ptr(), 999, 4, 1000, 5, p.data_ptr(), i.data_ptr()) == -1      # ld < N
    assert raw(None, 1000, 4, 1000, 5, p.data_ptr(), i.data_ptr()) == -1
    assert raw(z.data_ptr(), 1000, 4, 1000, 5, None, i.data_ptr()) == -1
    assert raw(z.data_ptr(), 1000, 4, 1000, 5, p.data_ptr(), None) == -1
    assert raw(z.data_ptr() + 2, 1000, 3, 1000, 5, p.data_ptr(), i.data_ptr()) == -1  # misaligned
    assert raw(z.data_ptr(), 1000, 0, 1000, 5, p.data_ptr(), i.data_ptr()) == -1
    assert raw(z.data_ptr(), 1000, 4, 0, 1, p.data_ptr(), i.data_ptr()) == -1
    torch.cuda.synchronize()
