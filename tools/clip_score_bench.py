"""CLIP-score throughput on one MI355X, ViT-B/32 shapes with random weights -> profiles/clip_score_bench.txt:
  * image tower (+ visual_projection) images/s at B = 64, fp32 and bf16 (graph replay, device events, warm-up first);
  * pdmk_image_prep_ex bicubic for 64 images of 512 x 512 -> 224 (device events);
  * end-to-end clip_score images/s over N seeded 512 x 512 `.npy` files with 8 DataLoader workers (wall clock);
  * transformers' CLIPModel image tower + projection, eager, on the same GPU (fp32 and fp16) as a same-box comparison.
Run: python tools/clip_score_bench.py [--files 1024] [--out profiles/clip_score_bench.txt]"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unlearn-ft_amd"))

import numpy as np
import torch


def timed(fn, warmup=3, iters=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_score_bench.txt"))
    args = ap.parse_args()
    from pdm import _pdmk
    from pdm.models.clip.clip_model import CLIPModel
    from pdm.models.clip.convert import TEXT_DEFAULTS, VISION_DEFAULTS
    from pdm.utils.clip_utils import clip_score, pack_images
    from pdm.utils.data import upload
    dev = torch.device("cuda:0")
    lines = [f"# tools/clip_score_bench.py on one {torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}; "
             f"ViT-B/32 shapes, random weights"]
    B = 64
    rng = np.random.default_rng(0)
    arrays = [rng.integers(0, 256, (512, 512, 3), dtype=np.uint8) for _ in range(B)]
    packed, desc = pack_images(arrays, 224)
    src, dev_desc = upload(packed, B, dev)
    pix = torch.empty(B, 3, 224, 224, device=dev)
    ms = timed(lambda: _pdmk.image_prep_ex(src, desc, dev_desc, pix, filter=1))
    lines.append(f"bicubic prep 64 x 512^2 -> 224: {ms:.3f} ms ({B / ms * 1e3:.0f} images/s)")
    models = {}
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        m = CLIPModel.from_configs(TEXT_DEFAULTS, VISION_DEFAULTS, 512, device=dev, dtype=dt, seed=1)
        models[name] = m
        ms = timed(lambda: m.encode_image(pix))
        lines.append(f"HIP image tower + projection B=64 {name}: {ms:.3f} ms ({B / ms * 1e3:.0f} images/s)")
        ids = torch.zeros(B, 77, dtype=torch.int64)
        ids[:, 0], ids[:, 1:9], ids[:, 9] = 49406, 320, 49407
        ms = timed(lambda: m.encode_text(ids))
        lines.append(f"HIP text tower + projection B=64 {name}: {ms:.3f} ms ({B / ms * 1e3:.0f} captions/s)")
    try:
        from transformers import CLIPConfig, CLIPModel as HFCLIP
        for name, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
            hf = HFCLIP(CLIPConfig(text_config=dict(TEXT_DEFAULTS), vision_config=dict(VISION_DEFAULTS),
                                   projection_dim=512)).eval().to(dev, dt)
            px = pix.to(dt)
            with torch.no_grad():
                ms = timed(lambda: hf.visual_projection(hf.vision_model(pixel_values=px).pooler_output))
            lines.append(f"transformers eager image tower + projection B=64 {name}: {ms:.3f} ms ({B / ms * 1e3:.0f} images/s)")
            del hf
    except Exception as e:                              # the comparison is optional; the HIP numbers stand on their own
        lines.append(f"transformers comparison skipped: {type(e).__name__}: {e}")
    with tempfile.TemporaryDirectory() as tmp:
        gi, tf = os.path.join(tmp, "gen"), os.path.join(tmp, "feat")
        os.makedirs(gi)
        os.makedirs(tf)
        for i in range(args.files):
            np.save(os.path.join(gi, f"{i:012d}.npy"), rng.integers(0, 256, (512, 512, 3), dtype=np.uint8))
            v = rng.standard_normal(512).astype(np.float32)
            np.save(os.path.join(tf, f"{i:012d}.npy"), v / np.linalg.norm(v))
        for name in ("fp32", "bf16"):
            clip_score(tf, gi, num_workers=8, batch_size=64, model=models[name])      # warm-up: graphs captured
            t0 = time.perf_counter()
            clip_score(tf, gi, num_workers=8, batch_size=64, model=models[name])
            dt_s = time.perf_counter() - t0
            lines.append(f"end-to-end clip_score {args.files} x 512^2 .npy, 8 workers, B=64 {name}: {dt_s:.2f} s "
                         f"({args.files / dt_s:.0f} images/s)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
