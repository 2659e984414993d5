"""Artist-erasure score (the reference's baselines/concept_prune/artist_erasure.py, utils/load_models.py and
benchmarking/benchmarking_utils.py): for every prompt of an artist one image of the *original* pruned checkpoint and one of the
*erased* model from the same initial latents, then CLIP's cos(prompt, image) of both - the mean / std of the erased images'
similarity and the share of prompts whose erased image is less similar to the prompt than the original one.

Host side (no GPU needed): the prompt CSV, the result path rules, the ESD checkpoint rewriting, the pairing of the image
files and the statistics.  GPU side: `load_pipelines` (which checkpoint a --baseline means; the models come from
pdm/utils/load_models.py), `generate` (two StableDiffusionPruningPipelines that share VAE, text encoder and tokenizer; the text
encoder runs once per prompt) and `score` (pdm/utils/clip_utils.py's decode / pack / prep, the HIP CLIP towers and
pdmk_cosine_pairs, one read-back at the end).  Nothing here imports pandas, diffusers or transformers' CLIPModel.
"""
import csv
import json
import logging
import os

import numpy as np
import torch

from .load_models import FrozenModels, golden_path

logger = logging.getLogger("pdm.erasure")

BASELINES = ("pdm", "pruned_baseline", "esd", "uce", "concept-prune")
BASELINES_NOT_BUILT = ("concept-ablation", "baseline")
GUIDANCE = 7.5


# ---- prompts
def default_prompts_csv(target):
    return golden_path("artist_prompts", f"test_{target}.csv")


def read_prompts(path):
    """The `prompt` column of the reference's datasets/test_<target>.csv, in file order.  `evaluation_seed` is read and
    ignored: the reference overwrites it with 0 (artist_erasure.py:102)."""
    prompts = []
    with open(path, encoding="utf-8", newline="") as f:
        for row in csv.DictReader(f):
            if "prompt" not in row or "evaluation_seed" not in row:
                raise ValueError(f"{path}: expected the columns `prompt` and `evaluation_seed`, got {sorted(k for k in row if k)}")
            int(row["evaluation_seed"])
            prompts.append(row["prompt"])
    if not prompts:
        raise ValueError(f"{path}: no prompts")
    return prompts


# ---- paths (artist_erasure.py:54-57, :165-166)
def check_baseline(baseline, ckpt_name=None):
    """`concept-prune` takes the checkpoint file scripts/baselines/concept_prune/save_union_over_time.py writes as
    --ckpt_name; without one the reference looks the target up in its table of checkpoint paths (utils/load_models.py),
    which is not built here."""
    if baseline in BASELINES_NOT_BUILT:
        raise NotImplementedError(f"--baseline {baseline}: not built here (built: {', '.join(BASELINES)})")
    if baseline == "concept-prune" and ckpt_name is None:
        raise NotImplementedError("--baseline concept-prune without --ckpt_name: the reference's table of checkpoint paths is "
                                  "not built here; pass the .pt file save_union_over_time.py wrote")
    if baseline not in BASELINES:
        raise ValueError(f"--baseline {baseline!r}: expected one of {', '.join(BASELINES + BASELINES_NOT_BUILT)}")


def _norm(path):
    return os.path.normpath(path).replace(os.sep, "/")


def model_component(model_id):
    """`model_id` as the reference joins it into the path, or its basename when it is an existing local path."""
    return os.path.basename(os.path.normpath(model_id)) if os.path.exists(model_id) else model_id


def run_ckpt(ckpt_name, original_ckpt):
    """The last two components of the normalised `ckpt_name or original_ckpt` (the reference's split('/')[-3:-1] of a path
    with a trailing slash)."""
    parts = _norm(ckpt_name if ckpt_name is not None else original_ckpt).split("/")
    return "/".join(parts[-2:])


def score_file_name(ckpt_name):
    p = os.path.basename(_norm(ckpt_name)).split(".pt")[0] if ckpt_name is not None else "concept-prune"
    return f"clip_scores_{p}_VG.json"


def result_root(result_dir, seed, res_path):
    if result_dir:
        return result_dir
    return f"results/results_seed_{seed}/" + res_path.split("/")[2]


def images_dir(args):
    """<root>/<model>/<target>/<baseline>/benchmarking/concept_erase/<run_ckpt>/concept_erase; with --sld_type the baseline
    component is <baseline>_SLD_<type>, so an SLD run never shares a directory with a plain one."""
    from .sld import with_suffix
    return os.path.join(result_root(args.result_dir, args.seed, args.res_path), model_component(args.model_id), args.target,
                        with_suffix(args.baseline, getattr(args, "sld_type", None)), "benchmarking", "concept_erase", run_ckpt(args.ckpt_name, args.original_ckpt),
                        "concept_erase")


# ---- erasure checkpoints (load_models.py:194-206, generate_fid_images.py:97-111)
def esd_state_dict(nested):
    """ESD's {module: {'weight': .., 'bias': ..}} -> {"<module>.weight": .., "<module>.bias": ..}, `unet.` removed from the
    module names."""
    st = {k.replace("unet.", ""): v for k, v in nested.items()}
    flat = {f"{k}.weight": v["weight"] for k, v in st.items() if "weight" in v}
    flat.update({f"{k}.bias": v["bias"] for k, v in st.items() if "bias" in v})
    return flat


def load_erasure_checkpoint(unet, path, esd=None):
    """esd (None: 'esd' in the path): the nested form, overlaid on the model's weights; otherwise a full state dict, loaded
    strictly."""
    logger.info("Loading erasure model from %s", path)
    st = torch.load(path, map_location="cpu")
    if ("esd" in path) if esd is None else esd:
        unet.overlay_state_dict(esd_state_dict(st))
    else:
        unet.load_state_dict(st)
    return unet


def erasure_dir_name(path):
    return path.replace("/", "_").replace(".", "_")


# ---- image pairs and statistics
def pair_files(directory, n):
    """[(original_i file, removal_i file)] for i < n, whatever clip_utils.load_image reads; a missing member raises."""
    from .clip_utils import IMAGE_EXTENSIONS, stem
    found = {}
    for name in sorted(os.listdir(directory)):
        ext = name.rsplit(".", 1)[-1].lower()
        if ext in IMAGE_EXTENSIONS or ext == "npy":
            found.setdefault(stem(name), os.path.join(directory, name))
    orig = [found.get(f"original_{i}") for i in range(n)]
    rem = [found.get(f"removal_{i}") for i in range(n)]
    n_o, n_r = sum(p is not None for p in orig), sum(p is not None for p in rem)
    if n_o != n or n_r != n:
        missing = [f"original_{i}" for i, p in enumerate(orig) if p is None] + [f"removal_{i}" for i, p in enumerate(rem) if p is None]
        raise ValueError(f"{directory}: {n} prompts, {n_o} original and {n_r} removal images (first missing: {missing[:3]})")
    return list(zip(orig, rem))


def statistics(sim_removed, flags):
    """artist_erasure.py:152-163 on Python lists, as the reference holds them."""
    similarity = [float(s) for s in sim_removed]
    scores = [int(f) for f in flags]
    return {"avg_similarity": float(np.mean(similarity)), "avg_score": float(np.mean(scores)),
            "std_similarity": float(np.std(similarity)), "std_score": float(np.std(scores))}


def write_result(directory, ckpt_name, results):
    path = os.path.join(directory, score_file_name(ckpt_name))
    with open(path, "w") as f:
        json.dump(results, f)
    return path


# ---- scoring (GPU)
@torch.no_grad()
def score_pairs(prompts, pairs, model, tokenizer, batch_size=64):
    """(sim_orig, sim_removed, flags) numpy arrays of length n: cos(prompt_i, original_i), cos(prompt_i, removal_i) in fp32
    and sim_removed < sim_orig as 0 / 1."""
    from .. import _pdmk
    from .clip_utils import load_image, pack_images, prep_images, tokenize
    n, dev, R = len(prompts), model.device, model.image_size
    out = torch.zeros(3, n, device=dev)                                  # one buffer, one read-back
    sim_o, sim_r, flags = out[0], out[1], out[2].view(torch.int32)
    bs = max(int(batch_size), 1)
    for s in range(0, n, bs):
        e = min(s + bs, n)
        ids = tokenize(tokenizer, prompts[s:e], context_length=model.context_length)
        txt = model.encode_text(ids)
        feats = []
        for side in (0, 1):
            packed, desc = pack_images([load_image(p[side]) for p in pairs[s:e]], R)
            feats.append(model.encode_image(prep_images(packed, desc, R, dev)))
        _pdmk.cosine_pairs(txt, feats[0], feats[1], sim_o[s:e], sim_r[s:e], flags[s:e])
    host = out.cpu().numpy()
    return host[0].copy(), host[1].copy(), host[2].view(np.int32).astype(np.int64)


def score(prompts, directory, clip_model, tokenizer=None, batch_size=64, dtype=torch.float32, device=None, model=None):
    """The scoring stage over the files of `directory`: the reference's four numbers."""
    from .clip_utils import _tokenizer_for
    pairs = pair_files(directory, len(prompts))
    tok = _tokenizer_for(clip_model, tokenizer)
    if model is None:
        from ..models.clip.clip_model import CLIPModel
        print(f"Loading CLIP model: {clip_model}")
        model = CLIPModel.from_pretrained(clip_model, dtype=dtype, device=device)
    _, sim_removed, flags = score_pairs(prompts, pairs, model, tok, batch_size)
    return statistics(sim_removed.tolist(), flags.tolist())


# ---- generation (GPU)
def image_resolution(model_id, fallback):
    """sample_size x 8 of <model_id>/unet/config.json (768 for SD-2.1: what `pipeline(prompt)` defaults to), else `fallback`."""
    path = os.path.join(str(model_id), "unet", "config.json")
    if os.path.exists(path):
        with open(path) as f:
            cfg = json.load(f)
        if cfg.get("sample_size"):
            return int(cfg["sample_size"]) * 8
    return int(fallback)


def load_pipelines(config, args, device):
    """(original, erased) pipelines sharing VAE, text encoder, tokenizer and scheduler settings."""
    models = FrozenModels(config, device)
    original = models.load_unet(args.original_ckpt)
    if args.baseline == "pdm":
        if args.ckpt_name is None:
            raise ValueError("--baseline pdm needs --ckpt_name (the fine-tuned checkpoint directory)")
        erased = models.load_unet(args.ckpt_name)
    elif args.baseline == "pruned_baseline":
        erased = original
    else:                                             # esd, uce, concept-prune
        if args.ckpt_name is None:
            raise ValueError(f"--baseline {args.baseline} needs --ckpt_name (the erasure checkpoint file)")
        erased = load_erasure_checkpoint(models.load_unet(args.original_ckpt), args.ckpt_name, esd=args.baseline == "esd")
    return models.pipeline(original), models.pipeline(erased)


@torch.no_grad()
def generate(prompts, directory, original, erased, seed, resolution, steps, sld=None):
    """original_{i}.jpg / removal_{i}.jpg for every prompt (artist_erasure.py:99-115): the initial latents are drawn once per
    prompt from Generator(device).manual_seed(seed) and the text encoder runs once; both pipelines get the same `latents` and
    embeddings.  uint8 as diffusers' numpy_to_pil (rounded), JPEG by Pillow's default save.  sld: generate_samples' Safe
    Latent Diffusion keywords (pdm/utils/sld.py sampling_kwargs) for the removal images; the concept is encoded once."""
    from PIL import Image
    dev = original.device
    f = original.vae_scale_factor
    C = original.unet.cfg.in_channels
    neg = original.text_encoder(original._tokenize([""]))[0]
    latents, embeds = [], []
    for prompt in prompts:
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        latents.append(torch.randn((1, C, resolution // f, resolution // f), device=dev, dtype=torch.float32, generator=gen))
        embeds.append(original.text_encoder(original._tokenize([prompt]))[0])
    safe = {}
    if sld is not None:
        safe = {k: v for k, v in sld.items() if k != "safety_concept"}
        safe["safety_concept_embeds"] = erased.text_encoder(erased._tokenize([sld["safety_concept"]]))[0]
    for name, pipe in (("original", original), ("removal", erased)):
        for i in range(len(prompts)):
            img = pipe(prompt_embeds=embeds[i], negative_prompt_embeds=neg, latents=latents[i], num_inference_steps=steps,
                       guidance_scale=GUIDANCE, height=resolution, width=resolution, output_type="u8_round",
                       **(safe if name == "removal" else {})).images[0]
            Image.fromarray(img).save(os.path.join(directory, f"{name}_{i}.jpg"))
