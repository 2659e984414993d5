"""Inputs and CPU oracles of the UCE debiasing tests (tests/test_uce_debias_host.py, test_uce_debias_kernels_gpu.py,
test_uce_debias_gpu.py): the reference's loops restated in a chosen precision from the method's description - the target of
one (old text, projection) block with its aliased running norm, mat1 inverse(mat2) of one projection, the outer loop's
bookkeeping, the token windows and CLIP's zero-shot head - and seeded inputs for the two kernels.  Nothing is recorded from the
reference's own module: it downloads its models when imported."""
import numpy as np
import torch

from uce_fixtures import distance  # noqa: F401  (the tests' distance measure is the UCE tests')

# ---- pdmk_uce_debias_delta cases
DELTA_P = [1, 3]
DELTA_Q = [1, 4]
DELTA_A = [1, 2, 3, 8]
DELTA_SEED = 5


def delta_layout(P, Q):
    """(row_seg, col_seg, m, ld): unequal row segments (2, 5 and 1 rows), widths 64, 5, 33, 64 of which only the first starts
    on a multiple of 4, three padding rows, six uncovered columns."""
    row_seg = [0, 5] if P == 1 else [0, 2, 7, 8]
    col_seg = [0, 33] if Q == 1 else [0, 64, 69, 102, 166]
    return row_seg, col_seg, row_seg[-1] + 3, col_seg[-1] + 6


def delta_case(P, Q, A, seed=DELTA_SEED):
    """(O [m, w], U [A, m, w], weights [P, A]) fp32: attribute projections correlated with O (the running norm matters), weights
    of both signs up to 0.5; with P = 3 the middle pair's weights are all zero."""
    row_seg, col_seg, m, _ld = delta_layout(P, Q)
    g = torch.Generator().manual_seed(1000 * seed + 100 * P + 10 * Q + A)
    w = col_seg[-1]
    O = torch.randn(m, w, generator=g)
    U = torch.randn(A, m, w, generator=g) + 0.5 * O
    wt = torch.rand(P, A, generator=g) - 0.5
    wt[0, 0] = 0.3
    if A > 1:
        wt[0, 1] = -0.2
    if P == 3:
        wt[1] = 0
    return O, U, wt


def reference_target(o, us, w):
    """The reference's target of one block, literally: `target` is an alias of the old text's projection and `+=` writes
    through it, so the norm that scales step j is that of the running target."""
    o_embs = o.clone()
    target = o_embs
    for j, u in enumerate(us):
        u = u / u.norm()
        target += (w[j] * o_embs.norm()) * u
    return target


def reference_debias_delta(O, U, weights, row_seg, col_seg, dtype):
    """(D, S) in `dtype`: D = target - O per block (rows from row_seg[-1] on zero) and S = sum_j |c_j U_j| with c_j = w_j
    ||T_j|| / ||U_j||, the magnitude the componentwise bound is stated in.  A zero U_j block is left out (the reference: NaN)."""
    O, U, weights = O.to(dtype), U.to(dtype), weights.to(dtype)
    D, S = torch.zeros_like(O), torch.zeros_like(O)
    for p, (r0, r1) in enumerate(zip(row_seg, row_seg[1:])):
        for c0, c1 in zip(col_seg, col_seg[1:]):
            o = O[r0:r1, c0:c1]
            t = o.clone()
            for j in range(U.shape[0]):
                u = U[j, r0:r1, c0:c1]
                if not bool(u.any()):
                    continue
                step = (weights[p, j] * t.norm()) * (u / u.norm())
                S[r0:r1, c0:c1] += step.abs()
                t += step
            D[r0:r1, c0:c1] = t - o
    return D, S


def delta_bound(D64, S64):
    """One fp32 rounding of an fp64 sum: 2^-24 |D| + 2^-40 sum_j |c_j U_j| (the second term is generous for the fp64 Gram
    matrix, square roots and A fused multiply-adds, all of which err at the 2^-53 level times small counts)."""
    return 2.0 ** -24 * D64.abs() + 2.0 ** -40 * S64


# ---- the windows and the closed form
def group_slices(n_old, n_new, length):
    """Literal: f = n - 2, far = max over the old text and all new ones, old[f_old : length - max(0, far - f_old)], new j
    [f_j : length - max(0, far - f_j)]."""
    f_old = n_old - 2
    f_new = [n - 2 for n in n_new]
    far = max(f_new + [f_old])
    return slice(f_old, length - max(0, far - f_old)), [slice(f, length - max(0, far - f)) for f in f_new]


def reference_debias_edit(W, groups, retains, weights, lamb, erase_scale, preserve_scale, dtype):
    """mat1 @ inverse(mat2) for one projection W [O, K] in `dtype`: groups = [(E_old rows, [E_att_j rows])] already sliced,
    weights[g] = that group's A weights, retains = [E_r [T, K]]; values from W as it is (the edit is progressive)."""
    W = W.to(dtype)
    mat1 = lamb * W
    mat2 = lamb * torch.eye(W.shape[1], dtype=dtype)

    def add(values, context, scale):
        nonlocal mat1, mat2
        cv = context.reshape(context.shape[0], context.shape[1], 1)
        cvt = context.reshape(context.shape[0], 1, context.shape[1])
        vv = values.reshape(values.shape[0], values.shape[1], 1)
        mat1 = mat1 + scale * (vv @ cvt).sum(dim=0)
        mat2 = mat2 + scale * (cv @ cvt).sum(dim=0)

    for (eo, eas), w in zip(groups, weights):
        eo = eo.to(dtype)
        target = reference_target(eo @ W.T, [ea.to(dtype) @ W.T for ea in eas], w.to(dtype))
        add(target, eo, erase_scale)
    for er in retains:
        er = er.to(dtype)
        add(er @ W.T, er, preserve_scale)
    return mat1 @ torch.inverse(mat2)


# ---- the outer loop's bookkeeping, literally (fp32 torch on the host)
def reference_schedule(ratios, retain_texts, old_texts, max_bias_diff=0.05, weight_step=0.1):
    """(done, weights, retain_texts, max_change) of one pass with the measured (bypass already applied) ratios."""
    desired = [torch.ones(len(r)) / len(r) for r in ratios]
    max_change = [(ratio - d).abs().max() for ratio, d in zip(ratios, desired)]
    if max(max_change) < max_bias_diff:
        return True, None, retain_texts, max_change
    delta = [weight_step * (d - ratio) for ratio, d in zip(ratios, desired)]
    delta = [delta[i] if mc > max_bias_diff else delta[i] * 0 for i, mc in enumerate(max_change)]
    add = [old_texts[i] for i, w in enumerate(delta) if w[0] == 0]
    ret = retain_texts
    if len(add) > 0:
        ret = ret + add
        ret = list(np.unique(ret))
    return False, delta, ret, max_change


# ---- CLIP's zero-shot head
GAP = 1e-3                       # the smallest top-2 gap of a row's cosines the mask is compared at


def zeroshot(img, txt, scale):
    """(logits fp32 [B, A] = fp32(scale cos) with cos in fp64 (a zero norm: 0), probs = torch's fp32 softmax of them,
    mask int32 = logit == row maximum, the row's top-2 gap of the fp64 cosines (inf with one class))."""
    x, t = img.double(), txt.double()
    den = x.norm(dim=1)[:, None] * t.norm(dim=1)[None, :]
    cos = torch.where(den > 0, (x @ t.T) / den, torch.zeros_like(den))
    logits = (float(np.float32(scale)) * cos).to(torch.float32)
    probs = torch.softmax(logits, dim=1)
    mask = (logits == logits.max(dim=1, keepdim=True)[0]).to(torch.int32)
    if cos.shape[1] > 1:
        top = cos.topk(2, dim=1)[0]
        gap = top[:, 0] - top[:, 1]
    else:
        gap = torch.full((cos.shape[0],), float("inf"), dtype=torch.float64)
    return logits, probs, mask, gap


def zeroshot_features(B, A, D, seed):
    """Seeded (img [B, D], txt [A, D]) fp32 whose every row has a top-2 cosine gap of at least GAP in the fp64 restatement: a
    row that falls short is drawn again (from the same generator) until it does not - no row is left out."""
    g = torch.Generator().manual_seed(seed)
    txt = torch.randn(A, D, generator=g)
    img = torch.randn(B, D, generator=g) * 3
    for _ in range(100):
        gap = zeroshot(img, txt, 1.0)[3]
        short = (gap < GAP).nonzero().flatten().tolist()
        if not short:
            return img, txt
        for b in short:
            img[b] = torch.randn(D, generator=g) * 3
    raise AssertionError("zeroshot_features: no draw with the gap")


def ulps(got, want):
    """|got - want| in units of want's fp32 spacing."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
