#!/usr/bin/env python3
"""UCE debiasing (the reference's baselines/unified-concept-editing/train-scripts/train_debias.py with its flags): measure, per
concept text, which attribute CLIP sees in the images the pruned checkpoint samples, and edit every cross-attention to_k / to_v
weight in closed form until the attributes are within 0.05 of uniform (pdm/utils/uce_debias.py).
    python scripts/baselines/unified_concept_editing/train_debias.py --concept "doctor, nurse" --attributes "male, female" \\
        --base_config_path CFG --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/ \\
        --clip_model <clip-vit-base-patch32 directory or ViT-B-32.pt>

* Texts (build_texts): per concept `image of c`, `photo of c`, `portrait of c`, `picture of c`, `c`; the class texts of each are
  that text with the concept replaced by every attribute; the retained texts are the professions of
  tests/golden/uce/professions.txt that are not being edited.  `--concept default0`: the 37 professions of
  configs/baselines/uce_debias.yaml, which also holds 0.05, the weight step 0.1, 30 iterations, 5 seeds and 20 steps.
* Measurement: per concept text and seed --num_images images (PNDM, guidance 7.5) at sample_size x 8 of
  <model_id>/unet/config.json (without that file --image_resolution), classified on the device; the 5 seeds of every outer
  iteration come from one np.random.RandomState(--seed).  --clip_model is resolved like clip_score.py's (a hub id raises
  FileNotFoundError); CLIP runs in fp32, --mixed_precision is the sampler's dtype.
* Writes <--output_dir>/models/unbiased-<name>.pt - the full U-Net state dict under the reference's key names, what
  `artist_erasure.py --baseline uce --ckpt_name` and `generate_fid_images.py --erasure_ckpt_path` load - and
  info/unbiased-<name>.txt: the old texts, the last weights, the first and the last ratios, one per line (the reference writes
  it under data/).  --base enters the name only; anything but 2.1 raises.
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import numpy as np
import torch

from pdm.utils import uce_debias as D
from pdm.utils.erasure_utils import image_resolution
from pdm.utils.load_models import FrozenModels, cuda_device, inference_config


def parse_args(argv=None):
    return D.add_arguments(argparse.ArgumentParser(prog="TrainUSD")).parse_args(argv)


def main(argv=None, settings=None):
    """settings: the dict of configs/baselines/uce_debias.yaml, when another than the file's is wanted (tests)."""
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    settings = settings or D.load_settings()
    old_texts, new_texts, retain_texts, name = D.build_texts(args.concept, args.attributes, None, args.base, settings)
    print(name)
    if args.ckpt_path is None:
        raise ValueError("--ckpt_path is required (the pruned checkpoint directory: arch_vector.pt + unet/)")
    from pdm.models.clip import convert
    from pdm.models.clip.clip_model import CLIPModel
    from pdm.utils.clip_utils import _tokenizer_for
    convert.resolve(args.clip_model)                      # a hub id raises here, before any model is built
    device = cuda_device(args.device)
    clip = CLIPModel.from_pretrained(args.clip_model, dtype=torch.float32, device=device)
    clip_tokenizer = _tokenizer_for(args.clip_model, args.tokenizer)
    config = inference_config(args.base_config_path, args.model_id, args.tiny, args.mixed_precision)
    models = FrozenModels(config, device)
    pipe = models.pipeline(models.load_unet(args.ckpt_path))
    weights, init_ratios, final_ratios, _iterations = D.debias_model(
        pipe, clip, clip_tokenizer, old_texts, new_texts, retain_texts, np.random.RandomState(args.seed),
        num_images=args.num_images, resolution=image_resolution(args.model_id, args.image_resolution), settings=settings)
    out = os.path.join(args.output_dir, "models", f"unbiased-{name}.pt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    torch.save(pipe.unet.state_dict(), out)
    os.makedirs(os.path.join(args.output_dir, "info"), exist_ok=True)
    with open(os.path.join(args.output_dir, "info", f"unbiased-{name}.txt"), "w") as fp:
        fp.write(str(old_texts) + "\n" + str(weights) + "\n" + str(init_ratios) + "\n" + str(final_ratios))
    print("Model saved at: ", out)
    return out


if __name__ == '__main__':
    main()
