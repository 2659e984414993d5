"""Writes tests/golden/fid_frechet.npz: seeded full-rank ReLU-like feature statistics and their Frechet distance by the scipy
TTUR form (pytorch-fid's calculate_frechet_distance: scipy.linalg.sqrtm(sigma1.dot(sigma2)), the 1e-6 diagonal retry when
the root is not finite, the imaginary part dropped) - the independent oracle of pdm.utils.fid_utils.frechet_distance, which
needs no scipy at run time.  Cases D = 64 / N = 500 and D = 256 / N = 2000 are stored; the D = 2048 / N = 6000 agreement is
printed into tests/golden/fid_frechet.report.txt only (its statistics would be 64 MB).  Needs scipy; run from the repository
root: python tools/make_fid_golden.py"""
import os
import sys

import numpy as np
from scipy import linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unlearn-ft_amd"))


def features(seed, n, d):
    """ReLU-like fp32 features with correlated dimensions: relu(z A + b), z ~ N(0, I)."""
    g = np.random.default_rng(seed)
    a = g.standard_normal((d, d)) / np.sqrt(d) + np.eye(d) * 0.5
    b = g.uniform(0.0, 0.6, d)
    return np.maximum(g.standard_normal((n, d)) @ a + b, 0).astype(np.float32)


def stats(f):
    f = f.astype(np.float64)
    return f.mean(axis=0), np.cov(f, rowvar=False)


def frechet_scipy(mu1, s1, mu2, s2, eps=1e-6):
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    if not np.isfinite(covmean).all():
        off = np.eye(s1.shape[0]) * eps
        covmean = linalg.sqrtm((s1 + off).dot(s2 + off))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))


def main():
    from pdm.utils.fid_utils import frechet_distance
    out, lines = {}, []
    for tag, d, n in (("d64", 64, 500), ("d256", 256, 2000), ("d2048", 2048, 6000)):
        mu1, s1 = stats(features(10 + d, n, d))
        mu2, s2 = stats(features(20 + d, n, d) * 1.1)
        ref = frechet_scipy(mu1, s1, mu2, s2)
        got = frechet_distance(mu1, s1, mu2, s2)
        lines.append(f"{tag}: D={d} N={n} scipy TTUR {ref!r} eigh form {got!r} relative difference {abs(got - ref) / abs(ref):.3e}")
        if d <= 256:
            out.update({f"{tag}_mu1": mu1, f"{tag}_sigma1": s1, f"{tag}_mu2": mu2, f"{tag}_sigma2": s2,
                        f"{tag}_fid": np.float64(ref)})
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "fid_frechet.npz"), **out)
    with open(os.path.join(gold, "fid_frechet.report.txt"), "w") as f:
        f.write(f"scipy {linalg.__name__} from scipy {__import__('scipy').__version__}, numpy {np.__version__}\n" + "\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
