"""Host-side data loading of the fine-tune / unlearn trainers: local COCO, cc3m or `datasets` directories -> batches of the
reference's schema (pdm/utils/data_utils.py:12-97, 112-135, 247-312; pdm/datasets/coco.py, cc3m.py):
`pixel_values` fp32 [B, 3, R, R] in [-1, 1] on the device, `input_ids` / `empty_input_ids` int64 [B, T] on the device (encoded
by the HIP CLIP text encoder inside the step, Trainer._prompt_embeds).

 * datasets: `get_dataset(config.data)` builds the train / validation splits as the reference does - COCO from
   `data_dir/images/train{year}` + `annotations/captions_train{year}.json`, cc3m from its split file and split directory,
   anything else from `dataset_name` (or `data_files`) as a LOCAL path read by `datasets`; there are no downloads, so a hub
   id raises FileNotFoundError;
 * workers (`data.dataloader.dataloader_num_workers`) decode the images with PIL (`convert("RGB")`, no JPEG draft / DCT
   scaling), pick the caption, tokenise it, draw the random crop / flip and pack the batch into one uint8 buffer: B image
   descriptors (pdmk_image_desc, include/pdmk.h) followed by the HWC images.  An image that fails to load is dropped;
   a batch left with none is empty (the trainer skips it, as the reference does);
 * the main process copies the (pinned) buffer to the device with one non-blocking copy and runs pdmk_image_prep on the
   current stream: resize, crop, flip and normalise in one launch, bit-exact with the reference's torchvision transform;
 * order: a permutation per epoch seeded from (seed, epoch); rank r of `world` takes every world-th entry of it (padded to a
   multiple of `world` by wrapping around, like DistributedSampler), so the shards are disjoint and every rank runs the
   same number of batches.  Caption, crop and flip draws come from a generator seeded from (seed, epoch, rank, batch):
   the same batches whatever the number of workers.
"""
import json
import math
import os

# this build never downloads: `datasets` / `transformers` are used on local paths only
os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

import numpy as np
import torch
from PIL import Image, ImageFile

# the reference's cc3m module sets this on import (pdm/datasets/cc3m.py:7), and with it for every dataset it loads
ImageFile.LOAD_TRUNCATED_IMAGES = True

DESC_BYTES = 64          # sizeof(pdmk_image_desc): eight int64


def _get(cfg, path, default=None):
    cur = cfg
    for part in path.split("."):
        if cur is None:
            return default
        cur = cur.get(part) if isinstance(cur, dict) else getattr(cur, part, None)
    return default if cur is None else cur


# ---- transform geometry (torchvision Resize(int) / CenterCrop / RandomCrop on a PIL image)
def resized_size(h, w, R):
    """(new_h, new_w): the short side becomes R, the long side int(R * long / short)."""
    if w <= h:
        return int(R * h / w), R
    return R, int(R * w / h)


def center_crop_origin(rh, rw, R):
    return int(round((rh - R) / 2.0)), int(round((rw - R) / 2.0))


# ---- the packed image batch: what the workers build, and its way to the device
def pack_images(arrays, rows):
    """uint8 [H, W, 3] arrays -> (packed, desc): one uint8 host buffer of B pdmk_image_desc, then the HWC images, each on a
    4-byte word, then one spare word (gaps and spare word zero); and the descriptors [offset, h, w, rh, rw, top, left,
    flip] as an int64 [B, 8] tensor.  rows: per image [h, w, rh, rw, top, left, flip], or a callable (h, w) -> (rh, rw,
    top, left, flip)."""
    for a in arrays:
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError(f"expected uint8 [H, W, 3] images, got {a.dtype} {a.shape}")
    if callable(rows):
        rows = [a.shape[:2] + tuple(rows(*a.shape[:2])) for a in arrays]
    B = len(arrays)
    d = np.zeros((B, 8), np.int64)
    off = 0
    for i, a in enumerate(arrays):
        d[i, 0], d[i, 1:] = off, rows[i]
        off += (a.size + 3) & ~3                     # every image starts on a 4-byte word
    head = B * DESC_BYTES
    packed = torch.empty(head + off + 4, dtype=torch.uint8)
    buf = packed.numpy()
    buf[:head] = d.reshape(-1).view(np.uint8)
    starts = d[:, 0].tolist() + [off]
    for i, a in enumerate(arrays):
        at = head + starts[i]
        buf[at:at + a.size] = a.reshape(-1)
        buf[at + a.size:head + starts[i + 1]] = 0
    buf[head + off:] = 0
    return packed, torch.from_numpy(d)


def upload(packed, B, device):
    """One non-blocking H2D copy of a packed batch of B images -> (the image bytes, the descriptors as an int64 view)."""
    buf = packed.to(device, non_blocking=True)
    head = B * DESC_BYTES
    return buf[head:], buf[:head].view(torch.int64)


def prep_nhwc(packed, desc, R, device, filter, mean, std):
    """Packed host batch -> normalised fp32 NHWC [B, R, R, 3] on the device: pdmk_image_prep_ex (resize, crop, / 255,
    (x - mean) / std), then pdmk_nchw_to_nhwc."""
    from .. import _pdmk
    B = desc.shape[0]
    src, dev_desc = upload(packed, B, device)
    pix = torch.empty(B, 3, R, R, device=device)
    _pdmk.image_prep_ex(src, desc, dev_desc, pix, filter=filter, mean=mean, std=std)
    x = torch.empty(B, R, R, 3, device=device)
    _pdmk.nchw_to_nhwc(pix, x, B, 3, R * R, 3)
    return x


# ---- datasets (pdm/utils/data_utils.py:12-65)
def load_coco_dataset(images_dir, annotations_file):
    """One row per caption annotation: (image path, caption); 2014 splits use COCO_<split>_%012d.jpg names."""
    from datasets import Dataset
    with open(annotations_file) as f:
        ann = json.load(f)["annotations"]
    split = os.path.basename(os.path.normpath(images_dir))
    pattern = f"COCO_{split}_%012d.jpg" if "2014" in images_dir else "%012d.jpg"
    return Dataset.from_dict({"image": [os.path.join(images_dir, pattern % a["image_id"]) for a in ann],
                              "caption": [a["caption"] for a in ann]})


def load_cc3m_dataset(data_dir, split="train", split_file="Train_GCC-training.tsv", split_dir="training"):
    """Images of `split_dir` named <row>_...; their captions are row <row> of the tab-separated split file."""
    import csv
    from datasets import Dataset
    with open(os.path.join(data_dir, split_file), newline="") as f:
        captions = [row[0] for row in csv.reader(f, delimiter="\t", quoting=csv.QUOTE_NONE)]
    names = sorted(os.listdir(os.path.join(data_dir, split_dir)))
    return Dataset.from_dict({"image": [os.path.join(data_dir, split_dir, n) for n in names],
                              "caption": [captions[int(n.split("_")[0])] for n in names]})


def load_local_dataset(name=None, data_files=None):
    """`datasets.load_dataset` on a local directory / file(s); a hub id is not available to this build."""
    from datasets import load_dataset, load_from_disk
    if data_files is not None:
        files = [data_files] if isinstance(data_files, str) else list(data_files)
        missing = [f for f in files if not os.path.exists(f)]
        if missing:
            raise FileNotFoundError(f"data_files {missing!r} do not exist (hub downloads are not available to this build)")
        ext = os.path.splitext(files[0])[1].lstrip(".")
        return load_dataset({"jsonl": "json", "tsv": "csv"}.get(ext, ext), data_files=files)
    if not name or not os.path.exists(name):
        raise FileNotFoundError(
            f"dataset {name!r} is not a local directory / file (hub downloads are not available to this build): pass a local "
            f"copy laid out like the hub's")
    if os.path.exists(os.path.join(name, "dataset_dict.json")) or os.path.exists(os.path.join(name, "state.json")):
        ds = load_from_disk(name)
        return ds if hasattr(ds, "keys") else {"train": ds}
    return load_dataset(name)


def get_dataset(data):
    """{"train": Dataset, "validation": Dataset or None} from the `data` section of the config."""
    data_dir = _get(data, "data_dir") or ""
    if "conceptual_captions" in data_dir:
        out = {"train": load_cc3m_dataset(data_dir, "train", _get(data, "train_data_file", "Train_GCC-training.tsv"),
                                          _get(data, "train_data_dir", "training")), "validation": None}
        if _get(data, "validation_data_dir") is not None:
            out["validation"] = load_cc3m_dataset(data_dir, "validation",
                                                  _get(data, "validation_data_file", "Validation_GCC-1.1.0-Validation.tsv"),
                                                  _get(data, "validation_data_dir"))
        return out
    if "coco" in data_dir:
        year = str(_get(data, "year", "2014"))
        train_year = "2014" if year == "2014_30k" else year
        out = {"train": load_coco_dataset(os.path.join(data_dir, "images", f"train{train_year}"),
                                          os.path.join(data_dir, "annotations", f"captions_train{train_year}.json"))}
        val_ann = os.path.join(data_dir, "annotations", f"captions_val{year}.json")
        out["validation"] = (load_coco_dataset(os.path.join(data_dir, "images", f"val{year}"), val_ann)
                             if os.path.exists(val_ann) else None)
        return out
    name = _get(data, "dataset_name")
    if name is None and _get(data, "data_files") is None:
        raise ValueError("Please provide a dataset name (data.dataset_name), a data.data_dir or data.data_files.")
    ds = dict(load_local_dataset(name, _get(data, "data_files")))
    if name and "parti-prompts" in name:
        ds["train"] = ds["train"].add_column("index", list(range(len(ds["train"]))))
        ds["validation"] = ds["train"]
    if "validation" not in ds:
        split = ds["train"].train_test_split(test_size=0.083333, seed=42)
        ds = {"train": split["train"], "validation": split["test"]}
    return {"train": ds["train"], "validation": ds["validation"]}


def limit(dataset, n):
    """max_train_samples / max_validation_samples: the first n rows."""
    return dataset if (dataset is None or n is None) else dataset.select(range(min(int(n), len(dataset))))


def load_tokenizer(root):
    """transformers.CLIPTokenizer from <pretrained_model_name_or_path>/tokenizer, local files only."""
    if not root or not os.path.isdir(os.path.join(root, "tokenizer")):
        raise FileNotFoundError(
            f"tokenizer: {os.path.join(str(root), 'tokenizer')!r} is not a local directory (hub downloads are not available "
            f"to this build); pass a local snapshot laid out like the hub's")
    from transformers import CLIPTokenizer
    return CLIPTokenizer.from_pretrained(root, subfolder="tokenizer", local_files_only=True)


def tokenize(tokenizer, captions):
    return tokenizer(list(captions), max_length=tokenizer.model_max_length, padding="max_length", truncation=True,
                     return_tensors="pt").input_ids


# ---- samples (data_utils.py:100-135, 247-283)
def pick_caption(caption, train, rng):
    """One random caption of a list when training, the first one otherwise (maybe_keep_random_caption)."""
    if isinstance(caption, str):
        return caption
    if isinstance(caption, (list, tuple, np.ndarray)):
        return caption[int(rng.integers(len(caption)))] if train else caption[0]
    raise ValueError("Caption column should contain either strings or lists of strings.")


def open_rgb(image):
    """A decoded RGB uint8 array [H, W, 3], or None when the image cannot be opened / decoded."""
    try:
        if isinstance(image, str):
            with Image.open(image) as im:
                return np.asarray(im.convert("RGB"), np.uint8)
        if isinstance(image, dict):                      # a `datasets` Image feature not decoded: {"bytes", "path"}
            import io
            src = io.BytesIO(image["bytes"]) if image.get("bytes") else image["path"]
            with Image.open(src) as im:
                return np.asarray(im.convert("RGB"), np.uint8)
        return np.asarray(image.convert("RGB"), np.uint8)
    except Exception:
        return None


class PackedBatches(torch.utils.data.Dataset):
    """Batch-level dataset run by the DataLoader workers: item b of the current plan -> one packed host batch."""

    def __init__(self, rows, *, resolution, tokenizer, image_column, caption_column, train, center_crop, random_flip, seed,
                 rank):
        self.rows, self.R, self.tokenizer = rows, int(resolution), tokenizer
        self.image_column, self.caption_column = image_column, caption_column
        self.train, self.center_crop, self.random_flip = train, center_crop, random_flip
        self.seed, self.rank = int(seed), int(rank)
        self.plan, self.epoch = [], 0
        self._empty_ids = None

    def __len__(self):
        return len(self.plan)

    def empty_ids(self):
        if self._empty_ids is None and self.tokenizer is not None:
            self._empty_ids = tokenize(self.tokenizer, [""])
        return self._empty_ids

    def __getitem__(self, b):
        R = self.R
        rng = np.random.default_rng([self.seed, self.epoch, self.rank, int(b)])
        images, geometry, captions, index = [], [], [], []
        for i in self.plan[b]:
            row = self.rows[int(i)]
            caption = pick_caption(row[self.caption_column], self.train, rng)
            a = open_rgb(row[self.image_column])
            if a is None:                               # dropped, as collate_fn drops samples whose image failed
                continue
            h, w = a.shape[:2]
            rh, rw = resized_size(h, w, R)
            if self.center_crop:
                top, left = center_crop_origin(rh, rw, R)
            else:
                top, left = int(rng.integers(rh - R + 1)), int(rng.integers(rw - R + 1))
            flip = int(self.train and self.random_flip and rng.random() < 0.5)
            geometry.append([h, w, rh, rw, top, left, flip])
            images.append(a)
            captions.append(caption)
            index.append(int(i))
        B = len(images)
        packed, desc = pack_images(images, geometry)
        out = {"packed": packed, "image_desc": desc, "index": torch.tensor(index, dtype=torch.int64), "captions": captions}
        if self.tokenizer is not None:
            ids = tokenize(self.tokenizer, captions) if B else torch.zeros(0, self.empty_ids().shape[1], dtype=torch.int64)
            out["input_ids"] = ids
            out["empty_input_ids"] = self.empty_ids().expand(B, -1).contiguous()
        return out


class ImageCaptionLoader:
    """Iterable of the trainer's batches with a length; each `iter()` is one epoch (the next one after the last)."""

    def __init__(self, rows, *, batch_size, resolution, tokenizer=None, num_workers=0, seed=43, rank=0, world=1, train=True,
                 center_crop=False, random_flip=False, image_column="image", caption_column="caption", device=None,
                 shuffle=True):
        if rows is None or len(rows) == 0:
            raise ValueError("the dataset has no rows")
        self.rows, self.bs, self.seed = rows, int(batch_size), int(seed)
        self.rank, self.world, self.num_workers, self.device, self.shuffle = int(rank), int(world), int(num_workers), device, shuffle
        self.epoch = 0
        self.ds = PackedBatches(rows, resolution=resolution, tokenizer=tokenizer, image_column=image_column,
                                caption_column=caption_column, train=train, center_crop=center_crop, random_flip=random_flip,
                                seed=seed, rank=rank)

    def shard_size(self):
        return -(-len(self.rows) // self.world)

    def __len__(self):
        return -(-self.shard_size() // self.bs)

    def epoch_indices(self, epoch):
        """This rank's dataset rows for `epoch`, in order."""
        n = len(self.rows)
        if self.shuffle:
            order = torch.randperm(n, generator=torch.Generator().manual_seed(self.seed * 100003 + int(epoch))).tolist()
        else:
            order = list(range(n))
        total = self.shard_size() * self.world
        order = order + order[:total - n]
        return order[self.rank::self.world]

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def host_batches(self):
        """One epoch of packed host batches (the worker side); advances the epoch."""
        idx = self.epoch_indices(self.epoch)
        self.ds.plan = [idx[k:k + self.bs] for k in range(0, len(idx), self.bs)]
        self.ds.epoch = self.epoch
        self.epoch += 1
        pin = self.device is not None and torch.device(self.device).type == "cuda"
        return torch.utils.data.DataLoader(self.ds, batch_size=None, shuffle=False, num_workers=self.num_workers,
                                           pin_memory=pin)

    def __iter__(self):
        for hb in self.host_batches():
            yield hb if self.device is None else to_device(hb, self.ds.R, self.device)


def to_device(hb, R, device):
    """One non-blocking H2D copy of the packed buffer, then pdmk_image_prep on the current stream."""
    from .. import _pdmk
    B = hb["image_desc"].shape[0]
    out = {k: v for k, v in hb.items() if k != "packed"}
    if B == 0:
        out["pixel_values"] = torch.empty(0, 3, R, R, device=device)
    else:
        src, dev_desc = upload(hb["packed"], B, device)
        pix = torch.empty(B, 3, R, R, device=device)
        _pdmk.image_prep(src, hb["image_desc"], dev_desc, pix)
        out["pixel_values"] = pix
    for k in ("input_ids", "empty_input_ids"):
        if k in out:
            out[k] = out[k].to(device, non_blocking=True)
    return out


class PromptBatches:
    """Prompt batches for image logging (data_utils.py:286-290, trainer.py:2543-2575): token ids on the device."""

    def __init__(self, prompts, tokenizer, batch_size, device):
        self.prompts, self.tokenizer, self.bs, self.device = list(prompts), tokenizer, max(1, int(batch_size)), device

    def __len__(self):
        return -(-len(self.prompts) // self.bs)

    def __iter__(self):
        for k in range(0, len(self.prompts), self.bs):
            p = self.prompts[k:k + self.bs]
            yield {"prompts": p, "input_ids": tokenize(self.tokenizer, p).to(self.device),
                   "empty_input_ids": tokenize(self.tokenizer, [""] * len(p)).to(self.device)}


def read_prompts(prompts, max_generated_samples=None):
    """data.prompts: a list of prompts, or [a text file with one prompt per line] / [a directory of such files]
    (trainer.py:416-434)."""
    prompts = [prompts] if isinstance(prompts, str) else list(prompts)
    if prompts and os.path.isfile(prompts[0]):
        with open(prompts[0]) as f:
            prompts = [line.strip() for line in f]
    elif prompts and os.path.isdir(prompts[0]):
        d, prompts = prompts[0], []
        for name in sorted(os.listdir(d)):
            if name.endswith(".txt"):
                with open(os.path.join(d, name)) as f:
                    prompts.extend(line.strip() for line in f)
    if max_generated_samples is not None:
        prompts = prompts[:int(max_generated_samples)]
    return prompts
