"""Inputs and CPU oracles of the ConceptPrune tests (tests/test_concept_prune_gpu.py, tests/test_concept_prune_host.py), written
with torch's own F.normalize, torch.norm and torch.sort(stable=True); see tests/golden/concept_prune/concept_prune.report.txt
for why no vector comes from the reference's own modules."""
import torch
import torch.nn.functional as F

ROWNORM_SHAPES = [(1, 8), (63, 72), (130, 72), (1025, 2568), (128, 5120)]
# (O, F, T, skill_ratio)
COUNT_CASES = [(5, 8, 2, 0.01), (40, 72, 3, 0.25), (40, 200, 3, 0.1), (24, 1000, 4, 0.01), (17, 5120, 2, 0.01),
               (3, 2568, 50, 0.01), (4, 72, 2, 1.0)]


# ---- pdmk_rownorm_colsq
def activations(M, Fd, seed, zero_rows=True):
    """fp32 [M, Fd] of bf16-representable values: row scales spread over 1e-3 ... 1e3, two all-zero rows (M >= 4)."""
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(M, 1, generator=g) * 6 - 3)
    x = (torch.randn(M, Fd, generator=g) * scale).to(torch.bfloat16).to(torch.float32)
    if zero_rows and M >= 4:
        x[M // 3] = 0
        x[M - 1] = 0
    return x


def colnorm_oracle(xs, dtype):
    """The reference's chain over the calls `xs`: norm <- sqrt(norm^2 + ||F.normalize(x, dim=1)||_col^2), in `dtype`."""
    norm = torch.zeros(xs[0].shape[1], dtype=dtype)
    for x in xs:
        new = torch.norm(F.normalize(x.to(dtype), dim=1), dim=0)
        norm = torch.sqrt(norm ** 2 + new ** 2)
    return norm


def rel_distance(got, ref64):
    """Largest relative distance from the fp64 oracle over the columns it is non-zero at (exact zeros must be met exactly)."""
    got, nz = got.double(), ref64 > 0
    assert torch.equal(got[~nz], ref64[~nz])
    return float(((got[nz] - ref64[nz]).abs() / ref64[nz]).max()) if nz.any() else 0.0


# ---- pdmk_wanda_count
def count_inputs(O, Fd, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(O, Fd, generator=g)
    nb = torch.rand(T, Fd, generator=g) + 0.1
    nt = nb * torch.exp(0.5 * torch.randn(T, Fd, generator=g))
    return w, nb, nt


def count_oracle(w, nb, nt, k, check_no_tie=False):
    """int32 [O, F]: sum over t of (f among the k largest |w| * nt[t] of its row, ties in ascending f) & (|w| nt[t] > |w| nb[t]).
    w: fp32 values of the weights.  check_no_tie: assert that the k-th and (k + 1)-th values differ in every row and t."""
    aw = w.to(torch.float32).abs()
    O, Fd = aw.shape
    count = torch.zeros((O, Fd), dtype=torch.int32)
    k = min(k, Fd)
    for t in range(nt.shape[0]):
        mt, mb = aw * nt[t], aw * nb[t]
        sel = torch.zeros((O, Fd), dtype=torch.bool)
        if k > 0:
            s = torch.sort(mt, dim=1, descending=True, stable=True)
            sel.scatter_(1, s.indices[:, :k], True)
            if check_no_tie and k < Fd:
                assert bool((s.values[:, k - 1] != s.values[:, k]).all())
        count += (sel & (mt > mb)).to(torch.int32)
    return count


def straddling_ties(w, nt, k):
    """Number of (t, row) whose k-th and (k + 1)-th largest scores are equal."""
    aw = w.to(torch.float32).abs()
    n = 0
    for t in range(nt.shape[0]):
        v = torch.sort(aw * nt[t], dim=1, descending=True, stable=True).values
        n += int((v[:, k - 1] == v[:, k]).sum())
    return n


def tie_inputs(O, Fd, T, k, dtype, seed=0):
    """count_inputs with, in every row, eight columns of equal weight and equal norms placed across the k-th place (four above,
    four below in index order), one row with only three non-zero weights, and eight columns with n_target == n_base."""
    w, nb, nt = count_inputs(O, Fd, T, seed)
    for t in range(1, T):                     # the same ranking at every t (powers of two: exact)
        nt[t] = nt[0] * 2.0 ** t
    cols = torch.arange(8) * (Fd // 8) + 3
    nt[:, cols] = nt[:, cols[:1]]
    nb[:, cols] = 0.5 * nt[:, cols]           # selected ties are counted
    others = torch.ones(Fd, dtype=torch.bool)
    others[cols] = False
    for o in range(O):
        u = torch.sort(w[o, others].abs() * nt[0, others], descending=True).values
        w[o, cols] = 0.5 * (u[k - 5] + u[k - 4]) / nt[0, cols[0]]       # k - 4 scores above the tie value
    w[1] = 0
    w[1, [5, 77, Fd - 2]] = torch.tensor([0.5, -2.0, 1.5])
    same = torch.arange(8) * (Fd // 8) + 11
    nt[:, same] = nb[:, same]
    w = w.to(dtype).to(torch.float32)
    return w, nb, nt
