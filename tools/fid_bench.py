"""FID pipeline timings on one MI355X (measured, not gated) -> profiles/fid_bench.txt:
resize of 64 x 512^2, the Inception at B = 64 (ms, images/s, fp32 TFLOP/s against the 157 peak, the slowest conv shapes),
pdmk_fid_accumulate, the two eigh of frechet_distance on the host, compute_statistics over 1024 seeded .npy files with 8
workers; as comparator only, the same network restated in torch (tests/fid_fixtures.py, MIOpen) on the same GPU.
Run from the repository root:  python tools/fid_bench.py [--out profiles/fid_bench.txt] [--files 1024]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "unlearn-ft_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

PEAK = 157.3


def timed(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fid_bench.txt"))
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    from pdm import _pdmk as k
    from pdm.models.inception.inception_v3 import InceptionV3FID
    from pdm.utils import fid_utils as fu
    from pdm.utils.data import upload
    import fid_fixtures as fx
    dev, B = torch.device("cuda:0"), args.batch
    lines = [f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, batch {B}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (512, 512, 3), generator=g, dtype=torch.uint8).numpy() for _ in range(B)]
    packed, desc = fu.pack_images(imgs)
    src, dev_desc = upload(packed, B, dev)
    x = torch.empty(B, 299, 299, 3, device=dev)
    ms = timed(lambda: k.resize_bilinear_u8(src, desc, dev_desc, x))
    say(f"pdmk_resize_bilinear_u8 {B} x 512^2 -> 299^2: {ms:.3f} ms ({(B * 512 * 512 * 3 + x.numel() * 4) / ms / 1e6:.0f} GB/s of image bytes in + floats out)")

    sd = fx.seeded_state_dict(0)
    model = InceptionV3FID(device=dev, init=False)
    model.load_state_dict(sd)
    macs = 0
    per = {}
    orig = model.conv

    def conv(xm, name, out=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = orig(xm, name, out)
        b.record()
        torch.cuda.synchronize()
        u = model.units[name]
        per.setdefault(name, []).append((a.elapsed_time(b), xm.B * y.H * y.W * u.co * u.k, (xm.B * xm.H * xm.W, u.ci, u.co, u.kh, u.kw, u.stride)))
        return y

    net_ms = timed(lambda: model.forward_nhwc(x), iters=5)
    model.conv = conv
    for _ in range(3):
        model.forward_nhwc(x)
    model.conv = orig
    macs = sum(v[-1][1] for v in per.values())
    conv_ms = sum(min(t for t, _, _ in v) for v in per.values())
    say(f"InceptionV3FID B={B}: {net_ms:.2f} ms, {B / net_ms * 1e3:.0f} images/s, {macs / B / 1e9:.2f} GMAC/image, "
        f"{2 * macs / net_ms / 1e9:.1f} fp32 TFLOP/s ({100 * 2 * macs / net_ms / 1e9 / PEAK:.0f} % of {PEAK}); conv launches alone "
        f"(each synchronised) {conv_ms:.2f} ms")
    say("slowest conv units (ms, TFLOP/s, [pixels in, Ci, Co, kh, kw, stride]):")
    for name, v in sorted(per.items(), key=lambda kv: -min(t for t, _, _ in kv[1]))[:5]:
        t = min(t for t, _, _ in v)
        say(f"  {name:28s} {t:7.3f} ms {2 * v[0][1] / t / 1e9:6.1f} TFLOP/s {list(v[0][2])}")
    groups = {}
    for name, v in per.items():
        shp = v[0][2]
        cls = f"{shp[3]}x{shp[4]}" + ("/s2" if shp[5] == 2 else "")
        e = groups.setdefault(cls, [0.0, 0])
        e[0] += min(t for t, _, _ in v)
        e[1] += v[0][1]
    say("by kernel geometry (summed ms, TFLOP/s): " + ", ".join(f"{c}: {t:.2f} ms {2 * m / t / 1e9:.1f}" for c, (t, m) in sorted(groups.items())))

    # comparator: the torch restatement on the GPU (MIOpen), NCHW fp32
    sdg = {n: v.to(dev) for n, v in sd.items()}
    tnet = fx.Net(sdg)
    xn = ((x.permute(0, 3, 1, 2) + 1) / 2).contiguous()
    with torch.no_grad():
        t_ms = timed(lambda: tnet(xn), iters=5, warm=3)
        diff = (tnet(xn) - model.forward_nhwc(x)).abs().max().item()
    say(f"comparator torch eager (MIOpen) B={B}: {t_ms:.2f} ms, {B / t_ms * 1e3:.0f} images/s; max abs feature difference {diff:.2e}")

    f = model.forward_nhwc(x)
    total = torch.zeros(2048, device=dev, dtype=torch.float64)
    outer = torch.zeros(2048, 2048, device=dev, dtype=torch.float64)
    ms = timed(lambda: k.fid_accumulate(f, total, outer))
    say(f"pdmk_fid_accumulate B={B} D=2048: {ms:.3f} ms ({2 * B * 2048 * 2049 / 2 / ms / 1e6:.1f} fp64 GFLOP/s of the triangle)")

    rng = np.random.default_rng(0)
    fe = np.maximum(rng.standard_normal((6000, 2048)) + 0.3, 0)
    s1, s2 = np.cov(fe[:3000], rowvar=False), np.cov(fe[3000:], rowvar=False)
    t0 = time.time()
    fu.frechet_distance(fe[:3000].mean(0), s1, fe[3000:].mean(0), s2)
    say(f"frechet_distance D=2048 on the host (two eigh, {torch.get_num_threads()} threads): {time.time() - t0:.2f} s")

    with tempfile.TemporaryDirectory() as d:
        for i in range(args.files):
            np.save(os.path.join(d, f"{i:05d}.npy"), imgs[i % B])
        t0 = time.time()
        fu.compute_statistics(d, model=model, batch_size=B, num_workers=8)
        dt = time.time() - t0
    say(f"compute_statistics {args.files} x 512^2 .npy, 8 workers: {dt:.2f} s, {args.files / dt:.0f} images/s (30 000 images: {30000 / (args.files / dt):.0f} s)")
    with open(args.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
