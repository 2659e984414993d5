#!/usr/bin/env python3
"""Regenerates tests/golden/perceptual_ref.npz (+ .report.txt): the style / content / total loss that the REFERENCE'S OWN code
gives for the three seeded 48 x 48 pairs of tests/perceptual_fixtures.py, on seeded VGG-19 weights.

    python tools/make_perceptual_golden.py --reference <checkout of the reference project>

Runs on a machine that has the reference checked out; CPU only, deterministic (single-threaded float32 / float64 torch), so
a rerun gives the same file bit for bit.  The reference's baselines/unified-concept-editing/eval-scripts/styleloss.py is read
at run time: `gram_matrix`, `ContentLoss`, `StyleLoss`, `Normalization`, `get_style_model_and_losses` and
`get_style_content_loss` are cut out of its syntax tree and executed here - the module itself cannot be imported (it imports
torchvision and builds a pretrained VGG at import).  They run on an nn.Sequential laid out like torchvision's
`vgg19().features` (up to features.13, so that the reference's trimming has something to trim) holding the fixtures' weights.
Only numbers are written: the three losses per pair in float32 (as the reference runs) and in float64, and the gaps between
them.  No program text of the reference is stored; weights and images are regenerated from seeds by the tests.
"""
import argparse
import ast
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perceptual_fixtures as fx  # noqa: E402

NAMES = ("gram_matrix", "ContentLoss", "StyleLoss", "Normalization", "get_style_model_and_losses", "get_style_content_loss")
SOURCE = os.path.join("baselines", "unified-concept-editing", "eval-scripts", "styleloss.py")


def reference_functions(reference):
    path = os.path.join(reference, SOURCE)
    with open(path, encoding="utf-8") as f:
        tree = ast.parse(f.read(), path)
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in NAMES]
    missing = sorted(set(NAMES) - {n.name for n in keep})
    if missing:
        raise SystemExit(f"{path}: {missing} not found")
    ns = {"torch": torch, "nn": nn, "F": F, "device": torch.device("cpu"),
          "content_layers_default": ['conv_4'], "style_layers_default": ['conv_1', 'conv_2', 'conv_3', 'conv_4', 'conv_5']}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def vgg_features(sd, dtype):
    """vgg19().features[:14] with the fixtures' weights."""
    layers, convs = [], {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256)}
    for i in range(14):
        if i in convs:
            conv = nn.Conv2d(*convs[i], kernel_size=3, padding=1)
            conv.weight.data.copy_(sd[f"features.{i}.weight"])
            conv.bias.data.copy_(sd[f"features.{i}.bias"])
            layers.append(conv)
        elif i in (4, 9):
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers.append(nn.ReLU(inplace=True))
    return nn.Sequential(*layers).to(dtype).eval()


def run(ns, sd, dtype):
    cnn = vgg_features(sd, dtype)
    mean, std = (torch.tensor(v, dtype=dtype) for v in (fx.IMAGENET_MEAN, fx.IMAGENET_STD))
    out = []
    for a, b in zip(*fx.golden_pairs()):
        original, edited = fx.to_tensor(a, 48, dtype), fx.to_tensor(b, 48, dtype)
        with redirect_stdout(io.StringIO()):
            s, c, t = ns["get_style_content_loss"](cnn, mean, std, content_img=original, style_img=original, input_img=edited)
        out.append([s.double().item(), c.double().item(), t.double().item()])
    return np.asarray(out, np.float64)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reference", required=True, help="checkout of the reference project")
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "perceptual_ref.npz"))
    args = p.parse_args(argv)
    torch.set_num_threads(1)
    import warnings
    warnings.filterwarnings("ignore")
    ns = reference_functions(args.reference)
    sd = fx.vgg_state_dict()
    ref32, ref64 = run(ns, sd, torch.float32), run(ns, sd, torch.float64)
    gap = np.abs(ref32 - ref64) / np.abs(ref64)
    re64 = fx.vgg_losses(sd, *fx.golden_pairs(), 48, torch.float64)
    a, b = fx.pairs(7, 3, 64)
    l32, l64 = (fx.lpips(fx.alexnet_state_dict(), fx.lin_state_dict(), a, b, 64, d) for d in (torch.float32, torch.float64))
    lgap = np.abs(l32 - l64) / np.abs(l64)
    np.savez(args.out, ref32=ref32, ref64=ref64, gap=gap, lpips_gap=lgap)
    lines = ["style / content / total of the reference's styleloss.py on the seeded fixtures (3 pairs, 48 x 48)", ""]
    for i in range(3):
        lines.append(f"pair {i}: float32 {ref32[i].tolist()}")
        lines.append(f"        float64 {ref64[i].tolist()}")
    lines += ["", f"relative distance float32 vs float64, max over the pairs: style {gap[:, 0].max():.2e}, content "
              f"{gap[:, 1].max():.2e}, total {gap[:, 2].max():.2e}",
              f"fixtures' restatement (float64) vs the reference's code (float64), max relative: "
              f"{(np.abs(re64 - ref64) / np.abs(ref64)).max():.2e}",
              f"LPIPS restatement at 64 x 64 (3 pairs), float32 vs float64, max relative: {lgap.max():.2e}"]
    with open(os.path.splitext(args.out)[0] + ".report.txt", "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
