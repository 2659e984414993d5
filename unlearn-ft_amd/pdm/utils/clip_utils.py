"""CLIP score of generated images against their captions (the reference's pdm/utils/clip_utils.py, same entry points and
defaults), on the HIP CLIP model (pdm/models/clip/clip_model.py):

 * `clip_features(captions_dir)`: one normalised fp32 text feature [D] per caption `.txt`, saved as
   `<dirname(captions_dir)>/<model tag>_clip_features/<stem>.npy`;
 * `clip_score(text_features_dir, gen_images_dir)`: logit_scale.exp() * mean_i cos(text_i, image_i) over the generated
   images (`.npy` uint8 [H, W, 3], as scripts/metrics/generate_fid_images.py writes them, or image files).

DataLoader workers read the images and pack each batch into one host buffer (descriptors + HWC bytes, as pdm/utils/data.py
packs the training batches); the main process copies it to the device once and runs CLIP's transform there
(pdmk_image_prep_ex: Resize(R, BICUBIC) + CenterCrop + Normalize(CLIP mean / std), bit-exact with Pillow), the image tower,
and the score head, which adds the batch's cosines to an fp64 accumulator on the device: one read-back at the end.
Captions are tokenised on the host with transformers' CLIPTokenizer from local files, laid out as clip.tokenize lays them
out: [SOT, tokens..., EOT, 0, ...], an error (naming the file) when longer than the context.
Pairing is by file stem, not by the position in two sorted listings as the reference pairs them: a missing or extra file
on either side is an error instead of a silent shift of every later pair.
"""
import os

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

import numpy as np
import torch

from . import data
from .data import center_crop_origin, open_rgb, resized_size

IMAGE_EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"}
TEXT_EXTENSIONS = {"txt"}


def default_workers(num_workers=None):
    if num_workers is not None:
        return int(num_workers)
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count()
    return min(n, 8) if n is not None else 0


def list_dir(path):
    """Non-hidden entries of `path`, sorted (the reference's _combine_without_prefix)."""
    return sorted(os.path.join(path, n) for n in os.listdir(path) if not n.startswith("."))


def stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def pair_by_stem(text_files, image_files):
    """[(stem, text file, image file)] in sorted stem order; ValueError naming the first few unmatched files."""
    t = {stem(p): p for p in text_files}
    im = {stem(p): p for p in image_files}
    no_text, no_image = sorted(set(im) - set(t)), sorted(set(t) - set(im))
    if no_text or no_image:
        raise ValueError(f"text features and images do not pair by name: {len(image_files)} images, {len(text_files)} text "
                         f"features; {len(no_text)} images without a text feature (first: {no_text[:3]}), {len(no_image)} "
                         f"text features without an image (first: {no_image[:3]})")
    return [(s, t[s], im[s]) for s in sorted(t)]


# ---- captions
def load_tokenizer(path):
    """transformers.CLIPTokenizer from a local directory (vocab.json + merges.txt there or in its tokenizer/ subfolder)."""
    from transformers import CLIPTokenizer
    if path and os.path.isdir(path):
        for d in (path, os.path.join(path, "tokenizer")):
            if os.path.exists(os.path.join(d, "vocab.json")):
                return CLIPTokenizer.from_pretrained(d, local_files_only=True)
    raise FileNotFoundError(f"no CLIP tokenizer (vocab.json + merges.txt) in {path!r}: an OpenAI .pt file has no vocabulary; "
                            f"pass --tokenizer DIR (a transformers CLIP directory or <SD snapshot>/tokenizer: the same "
                            f"49408-token BPE vocabulary)")


def tokenize(tokenizer, captions, names=None, context_length=77):
    """int64 [B, context_length]: [SOT, tokens..., EOT, 0, ...] as clip.tokenize lays them out; longer captions raise."""
    out = torch.zeros(len(captions), context_length, dtype=torch.int64)
    for i, c in enumerate(captions):
        ids = tokenizer(c)["input_ids"]
        if len(ids) > context_length:
            what = names[i] if names is not None else repr(c[:40])
            raise ValueError(f"{what}: caption is {len(ids)} tokens long, longer than the context length {context_length}")
        out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
    return out


class _CaptionBatches(torch.utils.data.Dataset):
    def __init__(self, files, batch_size, tokenizer, context_length):
        self.files, self.bs, self.tok, self.ctx = files, int(batch_size), tokenizer, context_length

    def __len__(self):
        return -(-len(self.files) // self.bs)

    def __getitem__(self, b):
        files = self.files[b * self.bs:(b + 1) * self.bs]
        texts = []
        for f in files:
            with open(f) as fp:
                texts.append(fp.read())
        return {"input_ids": tokenize(self.tok, texts, files, self.ctx), "names": [stem(f) for f in files]}


# ---- images
def load_image(path):
    """uint8 [H, W, 3]: a `.npy` array or a decoded image file."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{path}: expected a uint8 [H, W, 3] array, got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a)
    a = open_rgb(path)
    if a is None:
        raise ValueError(f"{path}: cannot decode the image")
    return a


def pack_images(arrays, R):
    """data.pack_images with CLIP's geometry: resize the short side to R, center crop R x R."""
    def geometry(h, w):
        rh, rw = resized_size(h, w, R)
        return (rh, rw) + center_crop_origin(rh, rw, R) + (0,)
    return data.pack_images(arrays, geometry)


class _ScoreBatches(torch.utils.data.Dataset):
    """Batch b of the (stem, text feature, image) pairs: packed images + the text features stacked."""

    def __init__(self, pairs, batch_size, R):
        self.pairs, self.bs, self.R = pairs, int(batch_size), int(R)

    def __len__(self):
        return -(-len(self.pairs) // self.bs)

    def __getitem__(self, b):
        part = self.pairs[b * self.bs:(b + 1) * self.bs]
        packed, desc = pack_images([load_image(im) for _, _, im in part], self.R)
        txt = np.stack([np.load(t).astype(np.float32).reshape(-1) for _, t, _ in part])
        return {"packed": packed, "image_desc": desc, "text": torch.from_numpy(txt)}


def prep_images(packed, desc, R, device):
    """Packed host batch -> CLIP pixel values fp32 [B, 3, R, R] on the device (one H2D copy, one kernel)."""
    from .. import _pdmk
    B = desc.shape[0]
    src, dev_desc = data.upload(packed, B, device)
    pix = torch.empty(B, 3, R, R, device=device)
    _pdmk.image_prep_ex(src, desc, dev_desc, pix, filter=1)
    return pix


# ---- models
def load_model(clip_model="ViT-B/32", dtype=torch.float32, device=None):
    from ..models.clip.clip_model import CLIPModel
    print(f"Loading CLIP model: {clip_model}")
    return CLIPModel.from_pretrained(clip_model, dtype=dtype, device=device)


def _tokenizer_for(clip_model, tokenizer):
    if tokenizer is not None and not isinstance(tokenizer, str):
        return tokenizer
    if tokenizer is None:
        from ..models.clip import convert
        try:
            tokenizer = convert.resolve(clip_model)
        except FileNotFoundError:
            tokenizer = None
    return load_tokenizer(tokenizer)


def features_dir(dataset_path, clip_model):
    from ..models.clip import convert
    return os.path.join(os.path.dirname(dataset_path), f"{convert.model_tag(clip_model)}_clip_features")


@torch.no_grad()
def clip_features(dataset_path, clip_model="ViT-B/32", num_workers=None, batch_size=64, tokenizer=None,
                  dtype=torch.float32, model=None):
    """Normalised text features of the captions in `dataset_path` -> <dirname>/<tag>_clip_features/<stem>.npy; returns
    that directory."""
    files = list_dir(dataset_path)
    if not files:
        raise ValueError(f"{dataset_path}: no files")
    ext = files[0].rsplit(".", 1)[-1].lower()
    if ext not in TEXT_EXTENSIONS:
        raise ValueError(f"{dataset_path}: clip_features encodes captions (.txt files); got .{ext} files - image features "
                         f"are computed inside clip_score")
    tok = _tokenizer_for(clip_model, tokenizer)
    model = model or load_model(clip_model, dtype)
    dev = model.device
    ds = _CaptionBatches(files, batch_size, tok, model.context_length)
    dl = torch.utils.data.DataLoader(ds, batch_size=None, shuffle=False, num_workers=default_workers(num_workers),
                                     pin_memory=True)
    save_path = features_dir(dataset_path, clip_model)
    os.makedirs(save_path, exist_ok=True)
    from .. import _pdmk
    print("Calculating CLIP Features:")
    for batch in dl:
        ids = batch["input_ids"].to(dev, non_blocking=True)
        f = model.encode_text(ids)
        B, D = f.shape
        fn = torch.empty(B, D, device=dev)
        _pdmk.clip_score_head(f, None, fn, None, None, B, D)
        fn = fn.cpu().numpy()
        for i, name in enumerate(batch["names"]):
            np.save(os.path.join(save_path, f"{name}.npy"), fn[i])
    print("CLIP Features saved successfully!")
    return save_path


@torch.no_grad()
def clip_score(real_path, fake_path, clip_model="ViT-B/32", num_workers=None, batch_size=64, dtype=torch.float32,
               model=None):
    """real_path: the text feature `.npy` files of clip_features; fake_path: the generated images.  Returns the score as a
    Python float: logit_scale.exp() * mean over the pairs of cos(text, image)."""
    from .. import _pdmk
    pairs = pair_by_stem(list_dir(real_path), list_dir(fake_path))
    if not pairs:
        raise ValueError(f"{fake_path}: no images")
    model = model or load_model(clip_model, dtype)
    dev, R = model.device, model.image_size
    ds = _ScoreBatches(pairs, batch_size, R)
    dl = torch.utils.data.DataLoader(ds, batch_size=None, shuffle=False, num_workers=default_workers(num_workers),
                                     pin_memory=True)
    acc = torch.zeros(1, device=dev, dtype=torch.float64)
    n = 0
    print("Calculating CLIP Score:")
    for batch in dl:
        pix = prep_images(batch["packed"], batch["image_desc"], R, dev)
        img = model.encode_image(pix)
        txt = batch["text"].to(dev, non_blocking=True)
        B, D = img.shape
        if txt.shape != (B, D):
            raise ValueError(f"text features are {tuple(txt.shape[1:])} wide, the model's image features {D}")
        _pdmk.clip_score_head(img, txt, None, None, acc, B, D)
        n += B
    score = float(torch.exp(model.logit_scale).item()) * acc.item() / n
    print(f"{clip_model.replace('/', '-')} CLIP Score: {score:.4f}")
    return score
