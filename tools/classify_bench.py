"""Object-erasure classifier throughput on one MI355X, ResNet-50 with seeded weights -> profiles/classify_bench.txt.  Every
figure is the median of 5 samples; images are in memory (no decoding, no disk):
  * `classify` images/s at 224 x 224 (512 x 512 uint8 sources, resize 232, crop 224), B = 250 (the reference's batch) and
    B = 8, wall clock with the host-side packing, the copy and the read-back; and the forward pass alone (device events);
  * the 16 conv3 launches of a B = 64, 224 x 224 pass with the residual fused (pdmk_conv2d_fwd_res, relu = 1) against the
    same convs through pdmk_conv2d_fwd (relu = 0) followed by a torch add_ + relu_ (device events), with the arithmetic of
    the 16 convs and the rate reached;
  * pdmk_softmax_topk at [250, 1000], k = 5 (device events).
Run: python tools/classify_bench.py [--out profiles/classify_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unlearn-ft_amd"))

import numpy as np
import torch

SAMPLES = 5


def device_ms(fn, warmup=2, iters=5):
    """Median over SAMPLES of the mean time of `iters` calls between two device events."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(SAMPLES):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out)


def wall_ms(fn, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(SAMPLES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_bench.txt"))
    args = ap.parse_args()
    from pdm import _pdmk as k
    from pdm.models.resnet import ResNet50Classifier
    dev = torch.device("cuda:0")
    model = ResNet50Classifier(device=dev, seed=0)
    lines = [f"# tools/classify_bench.py on one {torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}; ResNet-50, "
             f"seeded weights, fp32, median of {SAMPLES}"]
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (512, 512, 3), dtype=np.uint8) for _ in range(250)]
    for B in (250, 8):
        ms = wall_ms(lambda: model.classify(images[:B], topk=5, batch_size=B))
        lines.append(f"classify 512^2 -> 224^2 B={B}: {ms:.2f} ms wall ({B / ms * 1e3:.0f} images/s)")
        x = model.prep(images[:B])
        ms = device_ms(lambda: model.forward_nhwc(x))
        lines.append(f"forward_nhwc 224^2 B={B}: {ms:.3f} ms ({B / ms * 1e3:.0f} images/s)")
        del x

    # the 16 conv3 units at B = 64: (stage width, map side, blocks)
    B = 64
    cases, flops = [], 0
    for l, (wd, side, n) in enumerate(((64, 56, 3), (128, 28, 4), (256, 14, 6), (512, 7, 3)), start=1):
        for i in range(n):
            u = model.units[f"layer{l}.{i}.conv3"]
            wo, bo = model.offsets[u.name]
            M = B * side * side
            t = torch.randn(M, u.ci, device=dev).abs_()
            res = torch.randn(M, u.co, device=dev)
            cases.append((u, model.arena[wo:wo + u.co * u.k], model.arena[bo:bo + u.co], t, res, torch.empty(M, u.co, device=dev), side))
            flops += 2 * M * u.ci * u.co

    def fused():
        for u, w, b, t, res, y, side in cases:
            k.conv2d_fwd_res(t, u.ci, w, b, res, u.co, y, u.co, B, side, side, u.ci, u.co, 1, 1, 1, 0, 0, relu=True)

    def unfused():
        for u, w, b, t, res, y, side in cases:
            k.conv2d_fwd(t, u.ci, w, b, y, u.co, B, side, side, u.ci, u.co, 1, 1, 1, 0, 0, relu=False)
            y.add_(res).relu_()

    def conv_only():
        for u, w, b, t, res, y, side in cases:
            k.conv2d_fwd(t, u.ci, w, b, y, u.co, B, side, side, u.ci, u.co, 1, 1, 1, 0, 0, relu=True)

    f, un, co = device_ms(fused), device_ms(unfused), device_ms(conv_only)
    lines.append(f"16 conv3 launches B=64 224^2, residual fused (pdmk_conv2d_fwd_res): {f:.3f} ms "
                 f"({flops / 1e9:.1f} GFLOP, {flops / f / 1e9:.1f} TFLOP/s)")
    lines.append(f"16 conv3 launches B=64 224^2, pdmk_conv2d_fwd then torch add_ + relu_: {un:.3f} ms ({un / f:.2f} x the fused time)")
    lines.append(f"16 conv3 launches B=64 224^2, pdmk_conv2d_fwd + ReLU without a residual: {co:.3f} ms")

    z = torch.randn(250, 1000, device=dev) * 3
    p = torch.empty(250, 5, device=dev)
    j = torch.empty(250, 5, device=dev, dtype=torch.int32)
    ms = device_ms(lambda: k.softmax_topk(z, 5, p, j), warmup=5, iters=50)
    lines.append(f"pdmk_softmax_topk [250, 1000] k=5: {ms * 1e3:.1f} us")
    ms = device_ms(lambda: torch.topk(torch.softmax(z, 1), 5, dim=1), warmup=5, iters=50)
    lines.append(f"torch softmax + topk [250, 1000] k=5 (same GPU, for scale): {ms * 1e3:.1f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f_:
        f_.write(text)


if __name__ == "__main__":
    main()
