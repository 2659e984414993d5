"""Inputs and CPU oracles of the UCE tests (tests/test_uce_gpu.py, tests/test_uce_host.py): the reference's closed form
W' = mat1 inverse(mat2) restated in a chosen precision from the method's description (tests/golden/uce/uce.report.txt says why
nothing is recorded from the reference's own module), SPD test matrices, and the componentwise error bounds of Cholesky
factorisation and solve (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3 and 10.4)."""
import numpy as np
import torch

U64 = 2.0 ** -53

FACTOR_N = [1, 16, 63, 64, 65, 130, 200]
SOLVE_M = [1, 5, 77]
SYSTEM_N = [1, 64, 100, 130]


def gamma(k):
    """gamma_k = k u / (1 - k u) for fp64."""
    return k * U64 / (1 - k * U64)


# ---- SPD systems
def spd_matrix(n, seed, cond=1e6, lam=0.5):
    """fp64 A = lam I + G^T G with low-rank-plus-noise G: a few dominant directions put the largest eigenvalue near lam * cond,
    the noise keeps every other direction just above lam.  The fp64 Cholesky factorisation on the CPU succeeds."""
    g = torch.Generator().manual_seed(seed)
    r = max(1, min(n // 4, 8))
    low = torch.randn(3 * r, r, generator=g, dtype=torch.float64) @ torch.randn(r, n, generator=g, dtype=torch.float64)
    low = low * (lam * cond / max(float(torch.linalg.matrix_norm(low, 2)) ** 2, 1e-300)) ** 0.5
    noise = 0.05 * torch.randn(n, n, generator=g, dtype=torch.float64)
    G = torch.cat([low, noise])
    A = lam * torch.eye(n, dtype=torch.float64) + G.T @ G
    A = 0.5 * (A + A.T)
    torch.linalg.cholesky(A)
    return A


def rhs(m, n, seed):
    return torch.randn(m, n, generator=torch.Generator().manual_seed(seed))


def _ld(t):
    return t.detach().cpu().double().numpy().astype(np.longdouble)


def matmul_wide(a, b):
    """a @ b of extended-precision arrays: in extended precision up to a few hundred columns (the host's own rounding is then
    far below the bounds under test), in fp64 beyond (its rounding grows like sqrt(n) u against bounds of n u)."""
    if a.shape[1] <= 256:
        return a @ b
    return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.longdouble)


def factor_excess(A, L):
    """max over the lower triangle of |A - L L^T| / (gamma_{n+1} |L| |L|^T) (Thm 10.3: <= 1)."""
    n = A.shape[0]
    L = _ld(torch.tril(L))
    res = np.abs(_ld(A) - matmul_wide(L, L.T))
    bound = gamma(n + 1) * matmul_wide(np.abs(L), np.abs(L).T)
    low = np.tril(np.ones((n, n), dtype=bool))
    return float((res[low] / bound[low]).max())


def solve_excess(A, L, B, X64):
    """max of |B - X A| / (gamma_{3n+1} |X| (|L| |L|^T)) (Thm 10.4 row by row: <= 1); A is taken from its lower triangle."""
    n = A.shape[0]
    L, X = _ld(torch.tril(L)), _ld(X64)
    res = np.abs(_ld(B) - matmul_wide(X, _ld(torch.tril(A) + torch.tril(A, -1).T)))
    bound = gamma(3 * n + 1) * matmul_wide(np.abs(X), matmul_wide(np.abs(L), np.abs(L).T))
    return float((res / bound).max())


def mirror_gram(g):
    """The symmetric matrix held by the 64 x 64 upper-triangle tiles of a pdmk_fid_accumulate `outer`."""
    n = g.shape[0]
    t = torch.arange(n) // 64
    upper = t[:, None] <= t[None, :]
    return torch.where(upper, g, g.T)


# ---- the reference's closed form
def slices(n_old, n_new, length):
    """Rows of the old and the new text of a pair: f = n - 2 (the last word token), far = max(f_old, f_new),
    old[f_old : length - (far - f_old)], new[f_new : length - (far - f_new)]."""
    f_old, f_new = n_old - 2, n_new - 2
    far = max(f_old, f_new)
    return slice(f_old, length - (far - f_old)), slice(f_new, length - (far - f_new))


def reference_target(o, nv, technique):
    """The target V of one pair and one projection from O = E_old W^T and N = E_new W^T."""
    if technique == "tensor":
        u = o / o.norm()
        return nv - (u * nv).sum() * u
    return nv


def reference_edit(W, pairs, retains, lamb, erase_scale, preserve_scale, technique, dtype):
    """mat1 @ inverse(mat2) for one projection W [O, K] in `dtype`: pairs = [(E_old rows, E_new rows)] already sliced, retains =
    [E_r [T, K]].  The sums of outer products are formed as the reference forms them (batched [rows, O, 1] @ [rows, 1, K],
    summed over the rows)."""
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

    for eo, en in pairs:
        eo, en = eo.to(dtype), en.to(dtype)
        add(reference_target(eo @ W.T, en @ W.T, technique), eo, erase_scale)
    for er in retains:
        er = er.to(dtype)
        add(er @ W.T, er, preserve_scale)
    return mat1 @ torch.inverse(mat2)


def reference_delta(O, N, row_seg, col_seg, technique, dtype):
    """V - O per (pair, projection) block in `dtype`; rows from row_seg[-1] on are zero.  An all-zero O block gives V = N (the
    reference's u = O / ||O|| is NaN there)."""
    O, N = O.to(dtype), N.to(dtype)
    D = torch.zeros_like(O)
    for r0, r1 in zip(row_seg, row_seg[1:]):
        for c0, c1 in zip(col_seg, col_seg[1:]):
            o, nv = O[r0:r1, c0:c1], N[r0:r1, c0:c1]
            v = nv if not bool(o.any()) else reference_target(o, nv, technique)
            D[r0:r1, c0:c1] = v - o
    return D


def distance(got, ref64):
    """max |got - ref64| over every tensor of the two lists, relative to max |ref64|."""
    num = max(float((g.double() - r).abs().max()) for g, r in zip(got, ref64))
    return num / max(float(r.abs().max()) for r in ref64)
