"""Data fixtures built at run time for the loader tests (nothing is downloaded): JPEG images written by PIL, COCO caption
annotations, a `datasets` directory, a small CLIP tokenizer (byte-level vocabulary + a few merges) and a pruned checkpoint
beside a tokenizer-only snapshot."""
import json
import os

import numpy as np
from PIL import Image

T = 13          # token row length of the tiny text encoder (tokenizer model_max_length)


def _byte_symbols():
    """GPT-2 / CLIP byte-level BPE alphabet: printable bytes map to themselves, the rest to code points from 256 on."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + list(range(ord("\xae"), 256))
    extra = iter(range(256, 512))
    return [chr(b) if b in keep else chr(next(extra)) for b in range(256)]


def write_tokenizer(root):
    """<root>/tokenizer: the 256 byte-level symbols and their </w> forms, the two special tokens, five merges."""
    d = os.path.join(root, "tokenizer")
    os.makedirs(d, exist_ok=True)
    syms = _byte_symbols()
    merges = [("t", "h"), ("th", "e</w>"), ("a", "n"), ("an", "d</w>"), ("o", "f</w>")]
    vocab = syms + [s + "</w>" for s in syms] + ["".join(m) for m in merges] + ["<|startoftext|>", "<|endoftext|>"]
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump({t: i for i, t in enumerate(vocab)}, f)
    with open(os.path.join(d, "merges.txt"), "w") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in merges))
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump({"tokenizer_class": "CLIPTokenizer", "model_max_length": T, "bos_token": "<|startoftext|>",
                   "eos_token": "<|endoftext|>", "unk_token": "<|endoftext|>", "pad_token": "<|endoftext|>"}, f)
    return root


def write_pruned_checkpoint_tree(root, dev, yaml_name):
    """A snapshot directory (tokenizer only: VAE and text encoder are seeded), a pruned checkpoint directory (tiny U-Net at
    budget 0.6, fp32, seed 3) and the YAML: dict(root, snap, ck, yaml, sd = the saved state dict)."""
    import torch
    import yaml
    from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    snap = write_tokenizer(os.path.join(root, "snapshot"))
    cfg = UNetConfig.tiny()
    av = arch_vector_for_budget(cfg, 0.6, hw=16)[0]
    unet = UNet2DConditionModelPruned(cfg, av, dev, torch.float32, train=False, seed=3)
    ck = os.path.join(root, "logs", "checkpoint-2")
    unet.save_pretrained(os.path.join(ck, "unet"))
    torch.save(unet.arch_vector, os.path.join(ck, "arch_vector.pt"))
    path = os.path.join(root, yaml_name)
    with open(path, "w") as f:
        yaml.safe_dump({"seed": 43, "tiny": True, "pretrained_model_name_or_path": snap,
                        "model": {"prediction_model": {"prediction_type": "v_prediction", "resolution": 64, "gated_ff": True,
                                                       "ff_gate_width": 32, "random_init": True}},
                        "training": {"mixed_precision": "no"}}, f)
    return dict(root=root, snap=snap, ck=ck, yaml=path, sd=unet.state_dict())


def image(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    a[..., 1] = ((xx + yy) * 255 // max(h + w - 2, 1)).astype(np.uint8)
    return Image.fromarray(a, "RGB")


SIZES = [(48, 64), (64, 48), (40, 40), (37, 53), (80, 60), (45, 70), (64, 64), (50, 90), (70, 41), (33, 47)]


def write_coco(root, year="2017", n=10, corrupt=()):
    """<root>/coco/{images/train<year>, annotations/captions_train<year>.json}: n images, two captions each; the images
    listed in `corrupt` are not JPEGs."""
    base = os.path.join(root, "coco")
    split = f"train{'2014' if year == '2014_30k' else year}"
    img_dir = os.path.join(base, "images", split)
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(os.path.join(base, "annotations"), exist_ok=True)
    ann = []
    for i in range(n):
        name = (f"COCO_{split}_%012d.jpg" if "2014" in split else "%012d.jpg") % (i + 1)
        path = os.path.join(img_dir, name)
        if i in corrupt:
            with open(path, "wb") as f:
                f.write(b"not an image")
        else:
            h, w = SIZES[i % len(SIZES)]
            image(h, w, seed=i).save(path, quality=90)
        ann += [{"image_id": i + 1, "id": 2 * i, "caption": f"a photo of the thing {i}"},
                {"image_id": i + 1, "id": 2 * i + 1, "caption": f"the other caption and {i}"}]
    with open(os.path.join(base, "annotations", f"captions_{split}.json"), "w") as f:
        json.dump({"annotations": ann}, f)
    return base


def write_style_dataset(root, n=8, styles=("monet", "picasso"), caption_column="prompt"):
    """A `datasets` directory (save_to_disk) with image / <caption_column> / style columns."""
    from datasets import Dataset, Features, Image as DImage, Value
    rows = {"image": [image(*SIZES[(i + 3) % len(SIZES)], seed=100 + i) for i in range(n)],
            caption_column: [f"a painting {i}" for i in range(n)], "style": [styles[i % len(styles)] for i in range(n)]}
    ds = Dataset.from_dict(rows, features=Features({"image": DImage(), caption_column: Value("string"), "style": Value("string")}))
    path = os.path.join(root, "upper")
    ds.save_to_disk(path)
    return path
