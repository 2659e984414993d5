"""Debias-VL's calibration on the GPU (csrc/spd.hip pdmk_pair_gram_f64, then the existing pdmk_spd_factor_f64 /
pdmk_spd_solve_f64; pdm/utils/debias_vl.py factor_from_pairs / apply) against numpy fp64.

Inputs: z are normalised rows, the female row equal to the male row plus 0.3 randn before normalising; embeddings X = randn.

pdmk_pair_gram_f64: elementwise against a numpy fp64 restatement, bound 2 (pairs + 3) 2^-53 (|lam| [i == j] + |scale| sum_p
|delta_p[i] delta_p[j]|) - the fp64 summation bound of a chain of `pairs` FMAs, the scale and the diagonal term, doubled for the
oracle's own rounding.  Two launches are bit-equal.

Transformed embeddings X (lam M + I)^-1: against numpy's fp64 `solve`, bound 4 x d_ref (max-abs), d_ref the distance from that
fp64 result of the reference's own chain on the same inputs (debiasing_vl.py: the mean of the fp32 outer products, G = 500 M + I,
np.linalg.inv, `.float()`, an fp32 matmul), measured here and printed.  Condition: the transform moves X by at least 1000 x
the bound, so a kernel that returns its input cannot pass."""
import numpy as np
import pytest
import torch

LAM = 500.0
SHAPES = [(24, 1, 5), (72, 3, 20), (200, 37, 33), (1024, 80, 154)]          # (d, pairs, m)


def pairs_and_embeds(d, pairs, m, seed=0):
    """(z fp32 [2 * pairs, d], X fp32 [m, d]) on the host."""
    gen = torch.Generator().manual_seed(seed + d)
    male = torch.randn(pairs, d, generator=gen)
    female = male + 0.3 * torch.randn(pairs, d, generator=gen)
    z = torch.stack([male / male.norm(dim=1, keepdim=True), female / female.norm(dim=1, keepdim=True)], 1).reshape(2 * pairs, d)
    return z.contiguous(), torch.randn(m, d, generator=gen)


def gram64(z, scale, lam):
    """(A, bound) of the contract in numpy fp64."""
    delta = z[0::2].double().numpy() - z[1::2].double().numpy()
    pairs, d = delta.shape
    A = scale * (delta.T @ delta) + lam * np.eye(d)
    mag = abs(scale) * (np.abs(delta).T @ np.abs(delta)) + abs(lam) * np.eye(d)
    return A, 2 * (pairs + 3) * 2.0 ** -53 * mag


def reference_chain(z, X):
    """debiasing_vl.py on the same inputs: fp32 outer products summed into an fp64 matrix, mean, inverse, fp32 matmul."""
    e = z.numpy()
    pairs, d = e.shape[0] // 2, e.shape[1]
    M = np.zeros((d, d))
    for p in range(pairs):
        zi, zj = e[2 * p][:, None], e[2 * p + 1][:, None]
        M += zi @ zi.T + zj @ zj.T - zi @ zj.T - zj @ zi.T
    M /= pairs
    P = torch.tensor(np.linalg.inv(LAM * M + np.eye(d)))
    return torch.matmul(X, P.T.float())


def transform_case(d, pairs, m):
    """(z, X, fp64 solution, d_ref, how far the transform moves X) on the host."""
    z, X = pairs_and_embeds(d, pairs, m)
    G, _ = gram64(z, LAM / pairs, 1.0)
    want = np.linalg.solve(G, X.double().numpy().T).T
    d_ref = float(np.abs(reference_chain(z, X).double().numpy() - want).max())
    return z, X, want, d_ref, float(np.abs(want - X.double().numpy()).max())


@pytest.mark.gpu
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("d,pairs,m", SHAPES)
def test_pair_gram_against_fp64(dev, d, pairs, m, strided):
    from pdm import _pdmk as k
    z, _ = pairs_and_embeds(d, pairs, m)
    pad = 8 if strided else 0
    zbuf = torch.full((2 * pairs, d + pad), 7.0)
    zbuf[:, :d] = z
    zd = zbuf.to(dev)[:, :d]
    scale = LAM / pairs
    outs = []
    for _ in range(2):
        buf = torch.full((d, d + pad), -3.0, device=dev, dtype=torch.float64)
        k.pair_gram(zd, scale, 1.0, buf[:, :d])
        outs.append(buf)
    assert torch.equal(outs[0], outs[1])
    assert (outs[0][:, d:] == -3.0).all(), "columns past d are not written"
    got = outs[0][:, :d].cpu().numpy()
    want, bound = gram64(z, scale, 1.0)
    err = np.abs(got - want)
    print(f"d {d} pairs {pairs}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(got, got.T)
    # other scalars: lam and scale enter as stated
    k.pair_gram(zd, -0.25, 3.0, outs[1][:, :d])
    want, bound = gram64(z, -0.25, 3.0)
    assert (np.abs(outs[1][:, :d].cpu().numpy() - want) <= bound).all()


@pytest.mark.gpu
@pytest.mark.parametrize("d,pairs,m", SHAPES)
def test_transformed_embeddings_against_fp64_solve(dev, d, pairs, m):
    from pdm import _pdmk as k
    from pdm.utils import debias_vl as D
    z, X, want, d_ref, moved = transform_case(d, pairs, m)
    bound = 4 * d_ref
    zd, Xd = z.to(dev), X.to(dev)
    A = torch.empty(d, d, device=dev, dtype=torch.float64)
    info = torch.zeros(1, device=dev, dtype=torch.int32)
    k.pair_gram(zd, LAM / pairs, 1.0, A)
    k.spd_factor(A, info)
    assert int(info.item()) == 0
    got = torch.empty(m, d, device=dev)
    k.spd_solve(A, Xd, got)
    err = float(np.abs(got.cpu().double().numpy() - want).max())
    print(f"d {d} pairs {pairs} m {m}: d_ref {d_ref:.3e}  bound {bound:.3e}  kernel {err:.3e}  transform moves X by {moved:.3f}")
    assert moved >= 1000 * bound
    assert err <= bound
    # the host layer is the same chain
    factor = D.factor_from_pairs(zd, LAM)
    assert int(factor.info.item()) == 0 and torch.equal(torch.tril(factor.L), torch.tril(A))
    assert torch.equal(D.apply(factor, Xd), got)
    y = D.apply(factor, Xd.view(1, m, d).to(torch.bfloat16))
    assert y.shape == (1, m, d) and y.dtype == torch.bfloat16
