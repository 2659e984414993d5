"""Fixtures of the CLIP-score tests, built at run time from seeds (nothing is downloaded): CLIP configs, transformers-named
weights drawn from a CPU torch generator, a transformers-layout model directory written by hand (config.json +
model.safetensors + the tokenizer of tests/data_fixtures.py, whose vocabulary the tiny text tower uses: EOT is its largest
id), seeded uint8 images, fixed captions, and the Pillow-bicubic CLIP transform written out on the CPU."""
import json
import math
import os

import numpy as np
import torch

from data_fixtures import write_tokenizer

VOCAB = 519           # write_tokenizer: 512 byte symbols, 5 merges, <|startoftext|> = 517, <|endoftext|> = 518
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

CONFIGS = {
    # (text config, vision config, projection_dim)
    "tiny": (dict(vocab_size=VOCAB, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                  max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="quick_gelu"),
             dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=224,
                  patch_size=32, layer_norm_eps=1e-5, hidden_act="quick_gelu"), 64),
    "b32": (dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
                 max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="quick_gelu"),
            dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=12, image_size=224,
                 patch_size=32, layer_norm_eps=1e-5, hidden_act="quick_gelu"), 512),
}
SEEDS = {"tiny": 11, "b32": 12}

# the script test's set: 12 images (mixed sizes, 512 x 512 among them) and their captions
E2E_SIZES = [(512, 512), (256, 256), (300, 200), (200, 300), (512, 512), (240, 320), (224, 224), (100, 150), (768, 1024),
             (512, 384), (333, 257), (512, 512)]
E2E_CAPTIONS = ["a photo of the cat", "the dog and the ball", "a red car of the city", "an old man and the sea",
                "the tree", "a bowl of fruit and bread", "the mountain and the lake", "a small boat",
                "two birds of the forest", "the train and the station", "a cup of coffee", "the end of the day"]


def _layer_shapes(prefix, E, F):
    out = {}
    for n in ("q", "k", "v", "out"):
        out[f"{prefix}self_attn.{n}_proj.weight"] = (E, E)
        out[f"{prefix}self_attn.{n}_proj.bias"] = (E,)
    for n in ("layer_norm1", "layer_norm2"):
        out[f"{prefix}{n}.weight"], out[f"{prefix}{n}.bias"] = (E,), (E,)
    out[f"{prefix}mlp.fc1.weight"], out[f"{prefix}mlp.fc1.bias"] = (F, E), (F,)
    out[f"{prefix}mlp.fc2.weight"], out[f"{prefix}mlp.fc2.bias"] = (E, F), (E,)
    return out


def hf_shapes(text, vision, proj):
    """transformers CLIPModel parameter names -> shapes."""
    Et, Ev, p = text["hidden_size"], vision["hidden_size"], vision["patch_size"]
    npos = (vision["image_size"] // p) ** 2 + 1
    s = {"text_model.embeddings.token_embedding.weight": (text["vocab_size"], Et),
         "text_model.embeddings.position_embedding.weight": (text["max_position_embeddings"], Et),
         "text_model.final_layer_norm.weight": (Et,), "text_model.final_layer_norm.bias": (Et,),
         "vision_model.embeddings.class_embedding": (Ev,),
         "vision_model.embeddings.patch_embedding.weight": (Ev, 3, p, p),
         "vision_model.embeddings.position_embedding.weight": (npos, Ev),
         "vision_model.pre_layrnorm.weight": (Ev,), "vision_model.pre_layrnorm.bias": (Ev,),
         "vision_model.post_layernorm.weight": (Ev,), "vision_model.post_layernorm.bias": (Ev,),
         "visual_projection.weight": (proj, Ev), "text_projection.weight": (proj, Et), "logit_scale": ()}
    for i in range(text["num_hidden_layers"]):
        s.update(_layer_shapes(f"text_model.encoder.layers.{i}.", Et, text["intermediate_size"]))
    for i in range(vision["num_hidden_layers"]):
        s.update(_layer_shapes(f"vision_model.encoder.layers.{i}.", Ev, vision["intermediate_size"]))
    return s


def state_dict(tag):
    """Seeded transformers-named weights of CONFIGS[tag]: Linear / conv weights N(0, 1 / fan_in), embeddings N(0, 0.5^2),
    LayerNorm gains 1 + N(0, 0.1^2), biases N(0, 0.05^2), logit_scale = log(1 / 0.07)."""
    text, vision, proj = CONFIGS[tag]
    g = torch.Generator().manual_seed(SEEDS[tag])
    sd = {}
    for name, shape in sorted(hf_shapes(text, vision, proj).items()):
        if name == "logit_scale":
            sd[name] = torch.tensor(math.log(1 / 0.07))
        elif "embedding" in name:
            sd[name] = torch.randn(shape, generator=g) * 0.5
        elif "norm" in name and name.endswith(".weight"):
            sd[name] = 1 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            sd[name] = 0.05 * torch.randn(shape, generator=g)
        else:
            fan_in = int(np.prod(shape[1:]))
            sd[name] = torch.randn(shape, generator=g) / math.sqrt(fan_in)
    return sd


def text_ids(tag, n=5, seed=3):
    """[n, 77] ids: SOT, random tokens, EOT (the largest id) at varied positions, zero padding."""
    V = CONFIGS[tag][0]["vocab_size"]
    rng = np.random.default_rng(seed)
    ids = np.zeros((n, 77), np.int64)
    for i in range(n):
        L = [1, 5, 20, 60, 75][i % 5]
        ids[i, 0] = V - 2
        ids[i, 1:1 + L] = rng.integers(0, V - 2, L)
        ids[i, 1 + L] = V - 1
    return ids


def image_array(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    a[..., 0] = ((xx * 255) // max(w - 1, 1)).astype(np.uint8)           # edges and gradients alike
    a[..., 2] = (((xx // 7 + yy // 5) % 2) * 255).astype(np.uint8)
    return a


def model_images(n=4, seed=40):
    sizes = [(512, 512), (300, 200), (224, 224), (150, 100)]
    return [image_array(*sizes[i % len(sizes)], seed + i) for i in range(n)]


def clip_preprocess(a, R=224):
    """CLIP's transform on the CPU: PIL Resize(R, BICUBIC) of the short side, center crop (torchvision's rounding),
    ToTensor (x / 255), Normalize((x - mean) / std) in fp32 -> [3, R, R] float32."""
    from PIL import Image
    h, w = a.shape[:2]
    rh, rw = (int(R * h / w), R) if w <= h else (R, int(R * w / h))
    im = Image.fromarray(a, "RGB")
    if (rh, rw) != (h, w):
        im = im.resize((rw, rh), Image.BICUBIC)
    top, left = int(round((rh - R) / 2.0)), int(round((rw - R) / 2.0))
    im = im.crop((left, top, left + R, top + R))
    x = np.asarray(im, np.uint8).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    mean = np.asarray(CLIP_MEAN, np.float32).reshape(3, 1, 1)
    std = np.asarray(CLIP_STD, np.float32).reshape(3, 1, 1)
    return (x - mean) / std


def write_hf_dir(root, tag="tiny"):
    """<root>/clip-<tag>: config.json + model.safetensors (transformers CLIPModel layout) + vocab.json / merges.txt."""
    from safetensors.torch import save_file
    text, vision, proj = CONFIGS[tag]
    d = os.path.join(root, f"clip-{tag}")
    os.makedirs(d, exist_ok=True)
    V = text["vocab_size"]
    cfg = {"architectures": ["CLIPModel"], "model_type": "clip", "projection_dim": proj, "logit_scale_init_value": 2.6592,
           "text_config": dict(text, bos_token_id=V - 2, eos_token_id=V - 1, pad_token_id=V - 1, projection_dim=proj),
           "vision_config": dict(vision, num_channels=3, projection_dim=proj)}
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f, indent=1)
    save_file({k: v.contiguous() for k, v in state_dict(tag).items()}, os.path.join(d, "model.safetensors"))
    tok = write_tokenizer(os.path.join(root, f"tok-{tag}"))
    for n in ("vocab.json", "merges.txt", "tokenizer_config.json"):
        with open(os.path.join(tok, "tokenizer", n)) as fi, open(os.path.join(d, n), "w") as fo:
            fo.write(fi.read())
    return d


def write_e2e_tree(root):
    """<root>/annotations/captions_val2014_tiny.json (one caption per image), <root>/images/COCO_val2014_tiny_%012d.npy."""
    ann = os.path.join(root, "annotations")
    img = os.path.join(root, "images")
    os.makedirs(ann, exist_ok=True)
    os.makedirs(img, exist_ok=True)
    rows = []
    for i, ((h, w), cap) in enumerate(zip(E2E_SIZES, E2E_CAPTIONS)):
        rows.append({"image_id": i + 1, "id": i, "caption": cap})
        np.save(os.path.join(img, "COCO_val2014_tiny_%012d.npy" % (i + 1)), image_array(h, w, 500 + i))
    path = os.path.join(ann, "captions_val2014_tiny.json")
    with open(path, "w") as f:
        json.dump({"annotations": rows}, f)
    return path, img
