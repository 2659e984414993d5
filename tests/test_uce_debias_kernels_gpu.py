"""The two kernels of UCE debiasing (-m gpu): pdmk_uce_debias_delta against the fp64 restatement of the reference's in-place
target loop, and pdmk_zeroshot_head against the fp64 restatement of CLIP's zero-shot head (tests/uce_debias_fixtures.py).

Bounds.  Delta: componentwise |D - D64| <= 2^-24 |D64| + 2^-40 sum_j |c_j U_j| - one fp32 rounding of a sum formed in fp64,
from the kernel's contract, not from what it gives; the fp32 restatement of the same loop lies hundreds of times further out
(asserted: >= 4 x on at least one case), so the bound separates an fp64 evaluation from an fp32 one.  Head: masks and counts
exactly, on features whose every row has a top-2 cosine gap >= 1e-3 (chosen on the restatement); probabilities to 4 fp32 ulps of
torch's fp32 softmax of the same fp32 logits."""
import ctypes

import numpy as np
import pytest
import torch

import uce_debias_fixtures as fx

pytestmark = pytest.mark.gpu
SENTINEL = 1e4


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- pdmk_uce_debias_delta
def _delta_buffers(O, U, m, ld, dev):
    w = O.shape[1]
    bo = torch.full((m, ld), SENTINEL, device=dev)
    bu = torch.full((U.shape[0], m, ld), SENTINEL, device=dev)
    bd = torch.full((m, ld), SENTINEL, device=dev)
    bo[:, :w], bu[:, :, :w] = O.to(dev), U.to(dev)
    return bo, bu, bd


@pytest.fixture(scope="module")
def delta_oracles():
    """{(P, Q, A): (O, U, weights, D64, S64, excess of the fp32 restatement over the bound)}, computed once."""
    out = {}
    for P in fx.DELTA_P:
        for Q in fx.DELTA_Q:
            for A in fx.DELTA_A:
                row_seg, col_seg, _m, _ld = fx.delta_layout(P, Q)
                O, U, wt = fx.delta_case(P, Q, A)
                D64, S64 = fx.reference_debias_delta(O, U, wt, row_seg, col_seg, torch.float64)
                D32, _ = fx.reference_debias_delta(O, U, wt, row_seg, col_seg, torch.float32)
                bound = fx.delta_bound(D64, S64)
                nz = bound > 0
                out[(P, Q, A)] = (O, U, wt, D64, S64, float(((D32.double() - D64).abs()[nz] / bound[nz]).max()))
    return out


def test_delta_bound_is_not_empty(delta_oracles):
    excess = {key: v[5] for key, v in delta_oracles.items()}
    print("fp32 restatement / bound:", {key: round(v, 1) for key, v in excess.items()})
    assert max(excess.values()) >= 4


@pytest.mark.parametrize("A", fx.DELTA_A)
@pytest.mark.parametrize("Q", fx.DELTA_Q)
@pytest.mark.parametrize("P", fx.DELTA_P)
def test_uce_debias_delta(dev, delta_oracles, P, Q, A):
    from pdm import _pdmk as k
    row_seg, col_seg, m, ld = fx.delta_layout(P, Q)
    O, U, wt, D64, S64, _excess = delta_oracles[(P, Q, A)]
    w = col_seg[-1]
    bo, bu, bd = _delta_buffers(O, U, m, ld, dev)
    k.uce_debias_delta(bo[:, :w], bu[:, :, :w], bd[:, :w], wt.to(dev), row_seg, col_seg)
    out = bd.cpu()
    assert bool((out[:, w:] == SENTINEL).all())                       # the uncovered columns are untouched
    D = out[:, :w]
    assert bool((D[row_seg[-1]:] == 0).all())                         # the padding rows are zeroed
    err, bound = (D.double() - D64).abs(), fx.delta_bound(D64, S64)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"uce_debias_delta P = {P}, Q = {Q}, A = {A}: max |D - D64| / bound {worst:.3f}, max |D64| {float(D64.abs().max()):.3f}")
    assert bool((err <= bound).all())
    assert float(D64[:row_seg[-1]].abs().max()) > 0.05                # the weights move something
    if P == 3:                                                        # the pair whose weights are all zero: exact zeros
        assert not wt[1].any() and bool((D[row_seg[1]:row_seg[2]] == 0).all())
        assert bool((D[row_seg[0]:row_seg[1]] != 0).any())
    again = torch.full_like(bd, SENTINEL)
    k.uce_debias_delta(bo[:, :w], bu[:, :, :w], again[:, :w], wt.to(dev), row_seg, col_seg)
    assert torch.equal(_bits(again.cpu()), _bits(out))                # a fresh buffer, the same bits


@pytest.mark.parametrize("A", [2, 3])
def test_uce_debias_delta_zero_attribute_block_contributes_nothing(dev, A):
    from pdm import _pdmk as k
    P, Q = 3, 4
    row_seg, col_seg, m, ld = fx.delta_layout(P, Q)
    O, U, wt = fx.delta_case(P, Q, A)
    wt[1] = 0.25                                                       # every pair has weights here
    blk = (slice(row_seg[2], row_seg[3]), slice(col_seg[1], col_seg[2]))
    U = U.clone()
    U[(1,) + blk] = 0
    D64, S64 = fx.reference_debias_delta(O, U, wt, row_seg, col_seg, torch.float64)
    w = col_seg[-1]
    bo, bu, bd = _delta_buffers(O, U, m, ld, dev)
    k.uce_debias_delta(bo[:, :w], bu[:, :, :w], bd[:, :w], wt.to(dev), row_seg, col_seg)
    D = bd.cpu()[:, :w]
    assert bool(torch.isfinite(D).all())
    assert bool(((D.double() - D64).abs() <= fx.delta_bound(D64, S64)).all())
    assert bool((D[blk] != 0).any())                                  # the other attributes still move the block


def test_uce_debias_delta_rejects(dev):
    from pdm import _pdmk as k
    lib = k._lib
    m, ld, P, Q = 8, 16, 1, 1
    O, D = torch.zeros(m, ld, device=dev), torch.full((m, ld), SENTINEL, device=dev)
    U = torch.zeros(9, m, ld, device=dev)
    w = torch.zeros(P, 9, device=dev)
    seg = torch.tensor([0, 4, 0, 8], dtype=torch.int32).to(dev)
    ws = torch.zeros(64, device=dev, dtype=torch.float64)

    def call(A=2, o=None, u=None, d=None, wp=None, wsp=-1, ws_elems=64, P_=P):
        wsp = ws.data_ptr() if wsp == -1 else wsp
        return lib.pdmk_uce_debias_delta(o or O.data_ptr(), u or U.data_ptr(), d or D.data_ptr(), m, ld, A, wp or w.data_ptr(),
                                         seg.data_ptr(), P_, seg.data_ptr() + 8, Q, wsp, ws_elems, None)

    assert call() == 0
    torch.cuda.synchronize()
    assert bool((D[:, :8] == 0).all()) and bool((D[:, 8:] == SENTINEL).all())
    D.fill_(SENTINEL)
    for rc in (call(A=0), call(A=9), call(wsp=None), call(wsp=ws.data_ptr() + 4), call(o=O.data_ptr() + 2), call(u=U.data_ptr() + 1),
               call(d=D.data_ptr() + 2), call(wp=w.data_ptr() + 2), call(ws_elems=1), call(P_=65535)):
        assert rc == -1
    torch.cuda.synchronize()
    assert bool((D == SENTINEL).all())                                 # nothing was launched
    with pytest.raises(k.PdmkError):
        k.uce_debias_delta(O[:, :8], U[:, :, :8], D[:, :8], w, [0, 4], [0, 8])          # nine attributes
    with pytest.raises(k.PdmkError):
        k.uce_debias_delta(O[:, :8], U[:2, :, :8], D[:, :8], w[:, :3].contiguous(), [0, 4], [0, 8])   # weights of another A
    with pytest.raises(k.PdmkError):
        k.uce_debias_delta(O[:, :8], U[:2, :, :8], D[:, :8], w[:, :2].contiguous(), [0, 9], [0, 8])   # rows past m


# ---------------------------------------------------------------------------------------------- pdmk_zeroshot_head
SCALE = float(np.float32(np.exp(np.float32(np.log(1 / 0.07)))))


def _head(k, img, txt, dev, pad=8, **kw):
    """The head on features laid out with a row stride of D + pad."""
    bi = torch.full((img.shape[0], img.shape[1] + pad), 7.0, device=dev)
    bi[:, :img.shape[1]] = img.to(dev)
    return k.zeroshot_head(bi[:, :img.shape[1]], txt.to(dev), SCALE, **kw)


@pytest.mark.parametrize("D", [64, 100, 512])
@pytest.mark.parametrize("A", [1, 2, 5, 64])
@pytest.mark.parametrize("B", [1, 3, 70])
def test_zeroshot_head(dev, B, A, D):
    from pdm import _pdmk as k
    img, txt = fx.zeroshot_features(B, A, D, seed=B * 10000 + A * 100 + D)
    logits, probs64, mask64, gap = fx.zeroshot(img, txt, SCALE)
    assert bool((gap >= fx.GAP).all())                                # every row takes part
    hits = torch.zeros((1, A), device=dev, dtype=torch.int32)
    probs, mask = _head(k, img, txt, dev, hits=hits)
    assert probs.dtype == torch.float32 and mask.dtype == torch.int32 and tuple(probs.shape) == tuple(mask.shape) == (B, A)
    assert torch.equal(mask.cpu(), mask64)
    assert torch.equal(hits.cpu()[0], mask64.sum(0).to(torch.int32))
    assert bool((mask64.sum(1) == 1).all())
    u = fx.ulps(probs.cpu().numpy(), probs64.numpy())
    print(f"zeroshot_head B = {B}, A = {A}, D = {D}: probs within {u.max():.2f} ulp, smallest gap {float(gap.min()):.2e}")
    assert u.max() <= 4
    probs2, mask2 = _head(k, img, txt, dev)                           # no hits: the same bits
    assert torch.equal(_bits(probs2.cpu()), _bits(probs.cpu())) and torch.equal(mask2.cpu(), mask.cpu())


def test_zeroshot_head_duplicate_class_zero_row_and_groups(dev):
    from pdm import _pdmk as k
    B, A, D = 6, 4, 100
    img, txt = fx.zeroshot_features(B, A, D, seed=77)
    _l, _p, mask0, _g = fx.zeroshot(img, txt, SCALE)
    win = int(mask0[0].argmax())
    dup = (win + 1) % A
    txt[dup] = txt[win]                                                # row 0's winner exists twice
    img[4] = 0                                                         # a zero image row: cos = 0 everywhere
    logits, probs64, mask64, gap = fx.zeroshot(img, txt, SCALE)
    assert all(float(g) >= fx.GAP for g, row in zip(gap, mask64) if int(row.sum()) == 1)     # single winners win clearly
    assert int(mask64[0].sum()) == 2 and mask64[0, win] == 1 and mask64[0, dup] == 1
    assert mask64[4].tolist() == [1] * A and bool((probs64[4] == 0.25).all())
    group = torch.tensor([0, 3, 3, 0, 1, 3], dtype=torch.int32)         # group 2 stays empty
    hits = torch.zeros((4, A), device=dev, dtype=torch.int32)
    probs, mask = _head(k, img, txt, dev, group=group.to(dev), hits=hits)
    assert torch.equal(mask.cpu(), mask64)
    assert bool((probs.cpu()[4] == 0.25).all())
    want = torch.zeros((4, A), dtype=torch.int32)
    for b in range(B):
        want[group[b]] += mask64[b]
    assert torch.equal(hits.cpu(), want) and not want[2].any() and int(want[0, win]) >= 1 and int(want[0, dup]) >= 1
    _head(k, img, txt, dev, group=group.to(dev), hits=hits)             # a second launch accumulates
    assert torch.equal(hits.cpu(), 2 * want)
    # a group outside the table is left out of it
    hits3 = torch.zeros((3, A), device=dev, dtype=torch.int32)
    _head(k, img, txt, dev, group=group.to(dev), hits=hits3)
    assert torch.equal(hits3.cpu(), want[:3])


def test_zeroshot_head_rejects(dev):
    from pdm import _pdmk as k
    lib = k._lib
    B, A, D = 4, 3, 64
    img, txt = torch.randn(B, D, device=dev), torch.randn(A, D, device=dev)
    probs = torch.full((B, A), SENTINEL, device=dev)
    mask = torch.full((B, A), -7, device=dev, dtype=torch.int32)
    hits = torch.zeros((1, A), device=dev, dtype=torch.int32)

    def call(i=None, t=None, lda=D, ldb=D, B_=B, A_=A, D_=D, p=-1, mk=-1, h=None, G=0):
        return lib.pdmk_zeroshot_head(i or img.data_ptr(), lda, t or txt.data_ptr(), ldb, B_, A_, D_, ctypes.c_float(SCALE),
                                      probs.data_ptr() if p == -1 else p, mask.data_ptr() if mk == -1 else mk, None, h, G, None)

    for rc in (call(A_=0), call(A_=65), call(D_=0), call(D_=4097), call(B_=0), call(B_=65536), call(lda=D - 1), call(ldb=D - 1),
               call(p=None), call(mk=None), call(i=img.data_ptr() + 2), call(t=txt.data_ptr() + 1), call(h=hits.data_ptr(), G=0)):
        assert rc == -1
    torch.cuda.synchronize()
    assert bool((probs == SENTINEL).all()) and bool((mask == -7).all())   # nothing was launched
    assert call(h=hits.data_ptr(), G=1) == 0
    with pytest.raises(k.PdmkError):
        k.zeroshot_head(img, txt[:, :32], SCALE)                        # another width
    with pytest.raises(k.PdmkError):
        k.zeroshot_head(img.double(), txt, SCALE)
    with pytest.raises(k.PdmkError):
        k.zeroshot_head(img, txt, SCALE, group=torch.zeros(B, dtype=torch.int32, device=dev))      # group without hits
    with pytest.raises(k.PdmkError):
        k.zeroshot_head(img, txt, SCALE, hits=torch.zeros((1, A + 1), device=dev, dtype=torch.int32))
