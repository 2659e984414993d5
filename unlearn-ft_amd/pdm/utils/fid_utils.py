"""FID of a directory of generated images against stored real-image statistics: what the reference's scripts/metrics/fid.py
gets from clean-fid (`cleanfid.fid.compute_fid(gen_dir, dataset_name=..., mode="legacy_pytorch", dataset_split="custom")`
and `fid.make_custom_stats(name, dir, mode="legacy_pytorch")`), on the HIP Inception (pdm/models/inception).

clean-fid's `legacy_pytorch` mode, as restated in DESIGN 9c: every `.npy` (uint8 [H, W, 3]) or image file of the directory,
sorted; bilinear resize to 299 x 299 without antialiasing on the float image (not re-quantised); pytorch-fid's InceptionV3
pool3 features [N, 2048]; mu = mean, sigma = np.cov(rowvar=False) in float64; the Frechet distance of the two Gaussians.

DataLoader workers decode and pack each batch into one host buffer (descriptors + HWC bytes); the main process copies it to
the device once; resize, network and the fp64 sum / outer-product accumulation (pdmk_fid_accumulate) run there, and the
statistics are read back once at the end.  Nothing is ever downloaded: weights and statistics are local files.

`frechet_distance` needs no scipy: tr sqrtm(s1 s2) = sum_i sqrt(lambda_i(s1^1/2 s2 s1^1/2)) (the two products are similar
matrices), by two symmetric eigendecompositions in float64 on the CPU, negative eigenvalues (round-off of a positive
semi-definite matrix) clamped to 0.  On full-rank statistics it agrees with the scipy form pytorch-fid / clean-fid use
(`scipy.linalg.sqrtm(s1.dot(s2))`) to ~1e-13 relative; on rank-deficient ones (N < D) sqrtm turns singular and those packages
retry with 1e-6 added to both diagonals, while this form stays finite as it is - the two then differ by that regularisation.
"""
import os

import numpy as np
import torch

from .clip_utils import IMAGE_EXTENSIONS, default_workers, load_image
from . import data

MODES = ("legacy_pytorch",)
STATS_ENV = "PDM_FID_STATS"


# ---- host arithmetic
def _sym(a):
    return (a + a.T) * 0.5


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr(s1) + tr(s2) - 2 tr sqrtm(s1 s2) in float64 (a Python float)."""
    mu1, mu2 = (torch.as_tensor(np.asarray(m, np.float64)).reshape(-1) for m in (mu1, mu2))
    s1, s2 = (torch.as_tensor(np.asarray(s, np.float64)) for s in (sigma1, sigma2))
    D = mu1.numel()
    if mu2.numel() != D or tuple(s1.shape) != (D, D) or tuple(s2.shape) != (D, D):
        raise ValueError(f"statistics of different sizes: mu {mu1.numel()} / {mu2.numel()}, sigma {tuple(s1.shape)} / {tuple(s2.shape)}")
    lam, q = torch.linalg.eigh(_sym(s1))
    root = (q * lam.clamp_min(0).sqrt()) @ q.T                        # s1^1/2
    ev = torch.linalg.eigvalsh(_sym(root @ _sym(s2) @ root))
    tr_covmean = ev.clamp_min(0).sqrt().sum()
    diff = mu1 - mu2
    return float(diff @ diff + torch.trace(s1) + torch.trace(s2) - 2 * tr_covmean)


def finish_statistics(total, outer, n):
    """mu, sigma (float64 numpy) from sum_r x[r], the upper-triangle sum_r x[r] x[r]^T and the row count: np.mean / np.cov
    (divisor N - 1) in their one-pass form."""
    if n < 2:
        raise ValueError(f"statistics need at least 2 images, got {n}")
    total = torch.as_tensor(total, dtype=torch.float64).cpu()
    up = torch.triu(torch.as_tensor(outer, dtype=torch.float64).cpu())
    full = up + torch.triu(up, 1).T
    mu = total / n
    sigma = (full - n * torch.outer(mu, mu)) / (n - 1)
    return mu.numpy(), sigma.numpy()


# ---- files
def list_images(path):
    """Every `.npy` or image file under `path` (recursively), sorted."""
    out = []
    for root, _, names in os.walk(path):
        for n in names:
            ext = n.rsplit(".", 1)[-1].lower() if "." in n else ""
            if not n.startswith(".") and (ext == "npy" or ext in IMAGE_EXTENSIONS):
                out.append(os.path.join(root, n))
    return sorted(out)


def default_stats_dir():
    return os.environ.get(STATS_ENV) or os.path.join(os.path.expanduser("~"), ".cache", "pdm", "fid_stats")


def stats_path(name, mode="legacy_pytorch", stats_dir=None):
    """clean-fid's name of a custom statistics file: {name}_{mode}_custom_na.npz, lower case."""
    return os.path.join(stats_dir or default_stats_dir(), f"{name}_{mode}_custom_na.npz".lower())


def _check_mode(mode, split="custom"):
    if mode not in MODES:
        raise NotImplementedError(f"FID mode {mode!r}: only {MODES[0]!r} (the reference's) is implemented")
    if split != "custom":
        raise NotImplementedError(f"dataset_split {split!r}: only 'custom' statistics (make_custom_stats) are supported; "
                                  f"nothing is downloaded")


def save_stats(path, mu, sigma):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    np.savez_compressed(path, mu=np.asarray(mu, np.float64), sigma=np.asarray(sigma, np.float64))


def load_stats(path):
    with np.load(path) as z:
        return np.asarray(z["mu"], np.float64), np.asarray(z["sigma"], np.float64)


# ---- batches
def pack_images(arrays):
    """data.pack_images with the unused resize / crop fields as the identity: descriptors [offset, h, w, h, w, 0, 0, 0]."""
    return data.pack_images(arrays, lambda h, w: (h, w, 0, 0, 0))


def prep_images(packed, desc, device, size=299):
    """Packed host batch -> the network's input fp32 NHWC [B, size, size, 3] in [-1, 1] (one H2D copy, one kernel)."""
    from .. import _pdmk
    B = desc.shape[0]
    src, dev_desc = data.upload(packed, B, device)
    x = torch.empty(B, size, size, 3, device=device)
    _pdmk.resize_bilinear_u8(src, desc, dev_desc, x)
    return x


class _ImageBatches(torch.utils.data.Dataset):
    def __init__(self, files, batch_size):
        self.files, self.bs = files, int(batch_size)

    def __len__(self):
        return -(-len(self.files) // self.bs)

    def __getitem__(self, b):
        packed, desc = pack_images([load_image(f) for f in self.files[b * self.bs:(b + 1) * self.bs]])
        return {"packed": packed, "image_desc": desc}


def load_model(inception_weights=None, device=None):
    from ..models.inception.inception_v3 import InceptionV3FID
    return InceptionV3FID.from_pretrained(inception_weights, device=device)


@torch.no_grad()
def compute_statistics(path, model=None, inception_weights=None, batch_size=64, num_workers=None, return_features=False):
    """mu [D], sigma [D, D] (float64 numpy) of the Inception features of every image under `path`."""
    from .. import _pdmk
    files = list_images(path)
    if len(files) < 2:
        raise ValueError(f"{path}: {len(files)} images (.npy or image files); statistics need at least 2")
    model = model or load_model(inception_weights)
    dev = model.device
    dl = torch.utils.data.DataLoader(_ImageBatches(files, batch_size), batch_size=None, shuffle=False,
                                     num_workers=default_workers(num_workers), pin_memory=True)
    total = outer = None
    feats, n = [], 0
    for batch in dl:
        f = model.forward_nhwc(prep_images(batch["packed"], batch["image_desc"], dev))
        if total is None:
            D = f.shape[1]
            total = torch.zeros(D, device=dev, dtype=torch.float64)
            outer = torch.zeros(D, D, device=dev, dtype=torch.float64)
        _pdmk.fid_accumulate(f, total, outer)
        if return_features:
            feats.append(f.cpu())
        n += f.shape[0]
    mu, sigma = finish_statistics(total, outer, n)
    return (mu, sigma, torch.cat(feats).numpy()) if return_features else (mu, sigma)


def make_custom_stats(name, data_dir, mode="legacy_pytorch", stats_dir=None, **kw):
    """clean-fid's fid.make_custom_stats: the statistics of the real images -> {stats_dir}/{name}_{mode}_custom_na.npz."""
    _check_mode(mode)
    out = stats_path(name, mode, stats_dir)
    mu, sigma = compute_statistics(data_dir, **kw)
    save_stats(out, mu, sigma)
    print(f"saved custom FID statistics {out}")
    return out


def compute_fid(gen_dir, dataset_name, mode="legacy_pytorch", dataset_split="custom", stats_dir=None, **kw):
    """clean-fid's fid.compute_fid(gen_dir, dataset_name=..., mode=..., dataset_split="custom") as a Python float."""
    _check_mode(mode, dataset_split)
    ref = stats_path(dataset_name, mode, stats_dir)
    if not os.path.isfile(ref):
        raise FileNotFoundError(f"no FID statistics {ref}: make them from the real images with `python "
                                f"scripts/metrics/make_custom_stats.py --name {dataset_name} --data_dir REAL_IMAGES_DIR "
                                f"--mode {mode}` (or copy a clean-fid {os.path.basename(ref)} there)")
    mu2, sigma2 = load_stats(ref)
    mu1, sigma1 = compute_statistics(gen_dir, **kw)
    return frechet_distance(mu1, sigma1, mu2, sigma2)
