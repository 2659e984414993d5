#!/usr/bin/env python3
"""Entry point with the reference's name and flags (scripts/metrics/generate_fid_images.py:33-153): one uint8 image per
caption row of the validation split, sampled by a fine-tuned student, for FID / CLIP score.  Launch as
    python -m torch.distributed.run --nproc-per-node N scripts/metrics/generate_fid_images.py --base_config_path CFG \\
        --finetuning_ckpt_dir <logging_dir>/checkpoint-<step> [--mixed_precision bf16] [--image_resolution 512]

* Rows: `get_dataset(config.data)["validation"]` in dataset order; only the caption and image columns are read (the image
  files are never opened).  A batch holds image_generation_batch_size x world rows; rank r takes batches r, r + W, ...
  (accelerate's default sharding of the reference's DataLoader).  Deviation: every row is generated exactly once - a short
  last batch stays short, where accelerate pads it by wrapping around to the first rows.
* Models: `arch_vector.pt` and `unet/diffusion_pytorch_model.safetensors` of --finetuning_ckpt_dir (a trainer
  `checkpoint-N` directory as it is); block types from the config; VAE, CLIP text encoder and tokenizer from the snapshot
  (`pretrained_model_name_or_path`) under the trainer's `tiny` / `random_init` rules and dtype rule
  (`training.mixed_precision: null` -> fp32, as the reference): pdm/utils/load_models.py FrozenModels.
* Scheduler: PNDM from <snapshot>/scheduler/scheduler_config.json when present (values the class does not implement
  raise), else the SD-2.1 defaults with `model.prediction_model.prediction_type`.  Guidance 7.5; with `seed` set, a
  `torch.Generator(device).manual_seed(seed)` per batch, as the reference.
* Output: <finetuning_ckpt_dir>/<data.dataset_name>_fid_images_<training.num_inference_steps>/<image name>.npy, the image
  name being the last path component with a trailing ".jpg" removed; [R, R, 3] uint8 (R = --image_resolution, default 512)
  from pdmk_image_to_u8 (truncation, as `img * 255; img.astype(np.uint8)`).  Rows that share an image overwrite each other in
  row order.
* --erasure_ckpt_path FILE (generate_fid_images.py:97-111): an erasure baseline's checkpoint laid over the student's weights
  (pdm/utils/erasure_utils.py load_erasure_checkpoint: 'esd' in the path = ESD's nested {module: {weight, bias}} form,
  non-strict; otherwise a full state dict, strict).  The images then go to the reference's directory,
  <finetuning_ckpt_dir>/<path with '/' and '.' replaced by '_'>/<data.dataset_name>_fid_images/.
* --sld_type Weak|Medium|Strong|Max [--sld_concept TEXT, default the safety sentence of configs/baselines/sld.yaml]: the
  images are sampled with Safe Latent Diffusion on the selected checkpoint; the image directory's name gets `_SLD_<type>`
  appended.
* Ranks come from RANK / WORLD_SIZE / LOCAL_RANK; nothing collective runs on the GPU (a gloo barrier at the end), so
  several ranks may share one device.
"""
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch
import torch.distributed as dist

from pdm.utils.arg_utils import parse_args
from pdm.utils.config import load_config
from pdm.utils.erasure_utils import erasure_dir_name, load_erasure_checkpoint
from pdm.utils.load_models import FrozenModels, cuda_device
from pdm.utils.sld import sampling_kwargs, with_suffix

logger = logging.getLogger("pdm.generate_fid_images")
GUIDANCE = 7.5


def rank_batches(n_rows, batch, world, rank):
    """Row indices of the batches rank `rank` generates: batches of `batch` rows in dataset order, batch j to rank j % world."""
    return [list(range(s, min(s + batch, n_rows))) for j, s in enumerate(range(0, n_rows, batch)) if j % world == rank]


def image_file_name(image):
    """generate_fid_images.py:143-146: the last path component, a trailing ".jpg" removed, plus ".npy"."""
    if isinstance(image, dict) and image.get("path"):       # a `datasets` Image column read without decoding
        image = image["path"]
    name = str(image).split("/")[-1]
    if name.endswith(".jpg"):
        name = name[:-4]
    return name + ".npy"


def output_dir(config):
    name = config.get_path("data.dataset_name")
    sld_type = config.get("sld_type")
    if config.get("erasure_ckpt_path") is not None:
        return os.path.join(config.finetuning_ckpt_dir, erasure_dir_name(config.erasure_ckpt_path),
                            with_suffix(f"{name}_fid_images", sld_type))
    return os.path.join(config.finetuning_ckpt_dir,
                        with_suffix(f"{name}_fid_images_{config.get_path('training.num_inference_steps', 50)}", sld_type))


def validation_rows(config):
    """(captions, images) of the validation split in dataset order: the two columns only, images undecoded."""
    from pdm.utils import data as D
    ds = D.get_dataset(config.data)["validation"]
    if ds is None:
        raise ValueError("the dataset has no validation split")
    img_col = config.get_path("data.image_column", "image")
    capt_col = config.get_path("data.caption_column", "caption")
    ds = ds.select_columns([capt_col, img_col])
    feat = ds.features.get(img_col)
    if type(feat).__name__ == "Image":
        from datasets import Image
        ds = ds.cast_column(img_col, Image(decode=False))
    return [D.pick_caption(c, False, None) for c in ds[capt_col]], list(ds[img_col])


def main():
    args = parse_args()
    config = load_config(args.base_config_path)
    config.update(vars(args))                       # flat CLI overlay at the root, like the reference
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    assert config.finetuning_ckpt_dir is not None, "finetuning checkpoint directory must be provided"
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    device = cuda_device(local)
    seed = config.get("seed")
    if seed is not None:
        torch.manual_seed(int(seed))
    captions, images = validation_rows(config)
    logger.info("Dataset of size %d loaded.", len(captions))
    models = FrozenModels(config, device)
    unet = models.load_unet(config.finetuning_ckpt_dir)
    if config.get("erasure_ckpt_path") is not None:
        load_erasure_checkpoint(unet, config.erasure_ckpt_path)
    pipe = models.pipeline(unet)
    sld = {}
    if config.get("sld_type") is not None:
        sld = sampling_kwargs(config.sld_type, config.get("sld_concept"))
        sld["safety_concept_embeds"] = pipe.text_encoder(pipe._tokenize([sld.pop("safety_concept")]))[0]
    steps = int(config.get_path("training.num_inference_steps", 50))
    R = int(config.get("image_resolution") or 512)
    bs = int(config.get_path("data.dataloader.image_generation_batch_size", 1) or 1)
    out = output_dir(config)
    os.makedirs(out, exist_ok=True)
    for rows in rank_batches(len(captions), bs * world, world, rank):
        gen = None if seed is None else torch.Generator(device=device).manual_seed(int(seed))
        imgs = pipe(prompt=[captions[i] for i in rows], num_inference_steps=steps, guidance_scale=GUIDANCE, generator=gen,
                    output_type="u8", height=R, width=R, **sld).images
        for i, img in zip(rows, imgs):
            np.save(os.path.join(out, image_file_name(images[i])), img)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
