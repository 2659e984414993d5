"""Image-caption loader throughput (pdm/utils/data.py) and the pdmk_image_prep kernel alone.

Writes N seeded COCO-sized JPEGs (640 x 480 and 480 x 640, PIL, quality 90) plus a captions file into a temp dir, then
  * decode: PIL open + convert("RGB") per image in this process (the per-image host cost a worker pays),
  * loader: ImageCaptionLoader end to end (DataLoader workers decode / tokenise / pack, pinned H2D copy, the kernel on the
    current stream) at --workers workers, images/s over whole epochs after a warm-up epoch,
  * kernel: pdmk_image_prep on one packed batch of --batch COCO-sized images at --res, timed with HIP events.
Prints one JSON line per measurement.  bench.py does not use the loader.

    python tools/data_bench.py [--images 384] [--workers 16] [--batch 16] [--kernel_batch 8] [--res 512] [--epochs 2]
"""
import argparse
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unlearn-ft_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
from PIL import Image


def write_images(d, n, seed=0):
    rng = np.random.default_rng(seed)
    img_dir = os.path.join(d, "coco", "images", "train2017")
    os.makedirs(img_dir)
    os.makedirs(os.path.join(d, "coco", "annotations"))
    ann = []
    for i in range(n):
        h, w = (480, 640) if i % 3 else (640, 480)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        base = np.stack([128 + 100 * np.sin(xx / (17 + i % 11)), 128 + 100 * np.cos(yy / (23 + i % 7)),
                         (xx + yy) * 255 / (h + w)], -1)
        a = np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)      # photo-like: smooth plus grain
        Image.fromarray(a).save(os.path.join(img_dir, "%012d.jpg" % (i + 1)), quality=90)
        ann.append({"image_id": i + 1, "id": i, "caption": f"a photo of a thing number {i} on a table"})
    with open(os.path.join(d, "coco", "annotations", "captions_train2017.json"), "w") as f:
        json.dump({"annotations": ann}, f)
    return os.path.join(d, "coco")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=384)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--kernel_batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=2)
    args = ap.parse_args()
    import data_fixtures as F
    from pdm import _pdmk
    from pdm.utils import data as D
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        coco = write_images(d, args.images)
        tok = D.load_tokenizer(F.write_tokenizer(os.path.join(d, "snapshot")))
        rows = D.get_dataset({"data_dir": coco, "year": "2017"})["train"]
        print(json.dumps({"what": "fixture", "images": len(rows), "write_s": round(time.time() - t0, 2)}), flush=True)

        # decode alone, one process
        paths = rows["image"][:64]
        t0 = time.perf_counter()
        for p in paths:
            D.open_rgb(p)
        dec = (time.perf_counter() - t0) / len(paths)
        hb = D.PackedBatches(rows, resolution=args.res, tokenizer=tok, image_column="image", caption_column="caption",
                             train=True, center_crop=False, random_flip=True, seed=0, rank=0)
        hb.plan = [list(range(k, k + args.batch)) for k in range(0, 64, args.batch)]
        t0 = time.perf_counter()
        for b in range(len(hb.plan)):
            hb[b]
        pack = (time.perf_counter() - t0) / 64
        print(json.dumps({"what": "host_per_image_1proc", "decode_ms": round(dec * 1e3, 3),
                          "decode_tokenise_pack_ms": round(pack * 1e3, 3),
                          "decode_share": round(dec / pack, 3)}), flush=True)

        # loader end to end
        ld = D.ImageCaptionLoader(rows, batch_size=args.batch, resolution=args.res, tokenizer=tok, num_workers=args.workers,
                                  seed=0, random_flip=True, device=dev)
        for b in ld:                                   # warm-up epoch: worker start, page cache, first kernel launch
            pass
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        for _ in range(args.epochs):
            for b in ld:
                n += b["pixel_values"].shape[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"what": "loader", "workers": args.workers, "batch": args.batch, "res": args.res, "images": n,
                          "seconds": round(dt, 3), "images_per_s": round(n / dt, 1)}), flush=True)

        # the kernel alone on one packed batch
        ld1 = D.ImageCaptionLoader(rows, batch_size=args.kernel_batch, resolution=args.res, tokenizer=None, num_workers=0,
                                   seed=0, random_flip=True)
        hb = next(iter(ld1))
        B = hb["image_desc"].shape[0]
        src, dev_desc = D.upload(hb["packed"], B, dev)
        out = torch.empty(B, 3, args.res, args.res, device=dev)
        for _ in range(5):
            _pdmk.image_prep(src, hb["image_desc"], dev_desc, out)
        reps = 50
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            _pdmk.image_prep(src, hb["image_desc"], dev_desc, out)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        moved = src.numel() + out.numel() * 4
        print(json.dumps({"what": "kernel", "batch": B, "res": args.res, "ms": round(ms, 4), "MB_in": round(src.numel() / 1e6, 2),
                          "MB_out": round(out.numel() * 4 / 1e6, 2), "GB_per_s": round(moved / ms / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
