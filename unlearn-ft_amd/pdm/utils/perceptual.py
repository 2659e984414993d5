"""How much does an erasure change images it should have left alone: LPIPS (AlexNet) and the VGG-19 style / content loss of
the reference's baselines/unified-concept-editing/eval-scripts/lpips_eval.py and styleloss.py (the same files under
baselines/erasing/oldcode_erasing_compvis/eval-scripts), over two folders of `<case_number>_<n>.png` images sampled from the
original and from the edited model with the same seeds.  The trunks and metric heads are pdm/models/perceptual (pdmk_conv2d_fwd,
pdmk_lpips_layer, pdmk_gram_pair); this file is the host side: file matching, loading, batching, the CSVs.

* Many pairs per launch; the reference goes pair by pair.
* Images are uint8 [H, W, 3] arrays or paths read as `Image.open(...).convert("RGB")`; `Resize(imsize)` + `ToTensor` are
  pdmk_image_prep_ex with the bilinear filter, bit for bit.  Only SQUARE images are supported (the prep kernel crops to
  imsize x imsize; everything this project's samplers write is square): a non-square file raises ValueError naming it.
* Neither metric has been checked against the `lpips` / torchvision packages or their real weights: none of them is on the
  build machine.  The style / content loss is pinned to the reference's own code on seeded weights (tools/make_perceptual_golden.py),
  LPIPS to the formula of lpips v0.1 restated in tests/perceptual_fixtures.py.
"""
import csv
import math
import os

import numpy as np


# ---- names
def case_files(file_names, case_number):
    """The reference's matching: names containing `.png` that start with `<case_number>_` (so 1 does not take 10_0.png)."""
    return [f for f in file_names if ".png" in f and f.startswith(f"{case_number}_")]


def png_names(path):
    return sorted(n for n in os.listdir(path) if ".png" in n)


def result_basename(edited_path):
    """lpips_eval.py:86-89: the last component of --edited_path, the one before it when the path ends in a slash."""
    if len(os.path.basename(edited_path).strip()) == 0:
        return edited_path.split("/")[-2]
    return edited_path.split("/")[-1]


def result_csv(save_path, edited_path, kind):
    """<save_path>/<basename(edited_path)>_<kind>.csv, kind = lpipsloss / styleloss."""
    return os.path.join(save_path, f"{result_basename(edited_path)}_{kind}.csv")


# ---- images
def load_rgb(image):
    """uint8 [S, S, 3] of an array or a file; not square: ValueError naming it."""
    name = image if isinstance(image, str) else "array"
    if isinstance(image, str):
        from PIL import Image
        with Image.open(image) as im:
            a = np.asarray(im.convert("RGB"), np.uint8)
    else:
        a = np.ascontiguousarray(np.asarray(image))
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"{name}: expected a uint8 [H, W, 3] image, got {a.dtype} {a.shape}")
    if a.shape[0] != a.shape[1]:
        raise ValueError(f"{name}: {a.shape[1]} x {a.shape[0]} is not square; only square evaluation images are supported")
    return a


def _batched(images_a, images_b, model, imsize, batch_size):
    if len(images_a) != len(images_b):
        raise ValueError(f"{len(images_a)} originals against {len(images_b)} edited images")
    for i in range(0, len(images_a), int(batch_size)):
        a = [load_rgb(x) for x in images_a[i:i + batch_size]]
        b = [load_rgb(x) for x in images_b[i:i + batch_size]]
        yield model.forward_nhwc(model.prep(a, b, imsize))


def lpips_distance(images_a, images_b, model, imsize=64, batch_size=64):
    """LPIPS of every pair (a_i, b_i): float64 numpy [N].  model: AlexNetLPIPS."""
    out = [d.cpu().numpy() for d in _batched(images_a, images_b, model, imsize, batch_size)]
    return np.concatenate(out) if out else np.zeros(0)


def style_content_loss(originals, edited, model, imsize=512, batch_size=8):
    """(style, content, total) of every pair, each float64 numpy [N]; total = 1e6 style + content.  model: VGG19Style."""
    out = [[t.cpu().numpy() for t in r] for r in _batched(originals, edited, model, imsize, batch_size)]
    if not out:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    return tuple(np.concatenate([r[j] for r in out]) for j in range(3))


# ---- folders
def read_frame(csv_path):
    """(header, rows) of the prompts CSV; `case_number` is required."""
    with open(csv_path, encoding="utf-8", newline="") as f:
        rows = list(csv.reader(f))
    if not rows or "case_number" not in rows[0]:
        raise ValueError(f"{csv_path}: expected a `case_number` column, got {rows[0] if rows else []}")
    return rows[0], [r for r in rows[1:] if r]


def evaluate_folders(original_path, edited_path, csv_path, columns, metric):
    """The reference's loop.  Per row of the CSV: the files of original_path of its case; a file missing from edited_path is
    skipped and printed; `metric(originals, edited)` -> one array per column over all kept pairs (ONE call for the whole
    folder); the row gets the mean over its files, NaN without any.  Returns (header + columns, rows with the means appended)."""
    header, rows = read_frame(csv_path)
    ci = header.index("case_number")
    names = png_names(original_path)
    pairs, owner = [], []
    for r, row in enumerate(rows):
        for f in case_files(names, int(row[ci])):
            if not os.path.isfile(os.path.join(edited_path, f)):
                print(f"{f}: No File")
                continue
            pairs.append(f)
            owner.append(r)
    values = metric([os.path.join(original_path, f) for f in pairs], [os.path.join(edited_path, f) for f in pairs]) if pairs else ()
    values = [np.asarray(v, np.float64) for v in (values if isinstance(values, (tuple, list)) else (values,))]
    owner = np.asarray(owner, np.int64)
    out = []
    for r, row in enumerate(rows):
        sel = owner == r
        out.append(list(row) + [float(v[sel].mean()) if sel.any() else math.nan for v in values] if pairs
                   else list(row) + [math.nan] * len(columns))
    return header + list(columns), out


def write_frame(path, header, rows):
    """As DataFrame.to_csv: an unnamed index column first; floats with repr, NaN as `nan`."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + list(header))
        for i, row in enumerate(rows):
            w.writerow([i] + [repr(v) if isinstance(v, float) else v for v in row])
    return path
