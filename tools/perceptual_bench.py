#!/usr/bin/env python3
"""Times of the perceptual metrics on one GPU (seeded stand-in weights; the arithmetic does not depend on the values):
* LPIPS of 64 pairs at 64 x 64 (one batch) and style / content loss of 64 pairs at 512 x 512 (batches of 8), images already in
  memory as uint8 arrays: prep + trunk + metric heads, wall clock with a device synchronisation, median of --iters runs;
* pdmk_gram_pair alone on the 512 x 512, C = 64 map (conv_1 / conv_2 of the style loss) for B = 1 and 8: HIP-event time and
  the bytes of the two maps read once per second, next to the HBM rate a float4 copy reaches (6.3 TB/s).
    python tools/perceptual_bench.py [--out profiles/perceptual_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unlearn-ft_amd"))

from pdm import _pdmk as k  # noqa: E402
from pdm.models.perceptual import AlexNetLPIPS, VGG19Style  # noqa: E402
from pdm.utils import perceptual as P  # noqa: E402


def wall(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def events(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(ts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines = [f"perceptual_bench: {torch.cuda.get_device_name(0)}, {args.pairs} pairs, median of {args.iters}"]

    small = [rng.integers(0, 256, (64, 64, 3), dtype=np.uint8) for _ in range(2 * args.pairs)]
    alex = AlexNetLPIPS(device=dev)
    t = wall(lambda: P.lpips_distance(small[:args.pairs], small[args.pairs:], alex, imsize=64, batch_size=args.pairs), args.iters)
    lines.append(f"LPIPS 64 x 64, one batch: {t * 1e3:.2f} ms = {t / args.pairs * 1e6:.1f} us per pair")

    big = [rng.integers(0, 256, (512, 512, 3), dtype=np.uint8) for _ in range(2 * args.pairs)]
    vgg = VGG19Style(device=dev)
    t = wall(lambda: P.style_content_loss(big[:args.pairs], big[args.pairs:], vgg, imsize=512, batch_size=8), args.iters)
    lines.append(f"style / content 512 x 512, batches of 8: {t * 1e3:.1f} ms = {t / args.pairs * 1e3:.2f} ms per pair")

    HW, C = 512 * 512, 64
    for B in (1, 8):
        f = torch.randn(2 * B * HW, C, device=dev)
        ws = torch.empty(k.gram_workspace_elems(B, HW, C), device=dev)
        style = torch.zeros(B, device=dev, dtype=torch.float64)
        content = torch.zeros(B, device=dev, dtype=torch.float64)
        t = events(lambda: k.gram_pair(f, f[B * HW:], C, B, HW, C, ws, style, content), 4 * args.iters)
        nbytes = 2 * B * HW * C * 4
        lines.append(f"gram_pair HW = 512 x 512, C = 64, B = {B}: {t * 1e6:.1f} us for {nbytes / 1e6:.0f} MB of maps = "
                     f"{nbytes / t / 1e12:.2f} TB/s (achievable HBM copy rate 6.3 TB/s); workspace {ws.numel() * 4 / 1e6:.1f} MB")
        del f, ws
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
