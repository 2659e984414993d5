#!/usr/bin/env python3
"""Unified Concept Editing (the reference's baselines/unified-concept-editing/train-scripts/train_erase.py with its flags): the
closed-form edit of every cross-attention to_k / to_v weight of the pruned checkpoint.
    python scripts/baselines/unified_concept_editing/train_erase.py --concepts "Van Gogh" --guided_concepts art \\
        --concept_type art --base_config_path CFG --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/

* Texts (pdm/utils/uce.py build_texts): the concepts, with --add_prompts five templates each for `art` / `object`; the guiding
  texts (none: ' '); the retained texts [''] + --preserve_concepts, for --concept_type art by default every artist of
  tests/golden/uce/artists1734.txt that is not being erased (--preserve_number samples them, `<N>artists` samples the concepts;
  both on random.Random(--seed)).  The fixed lists allartist, i2g, 10artists and imagenette raise.
* Edit (edit_model): lam 0.5, --erase_scale 1, --preserve_scale max(0.1, 1 / retained texts); text encoder and weights in fp32
  whatever the settings file says; every distinct text is encoded once.
* Writes <--output_dir>/models/erased-<name>.pt - the full U-Net state dict under the reference's key names, fp32, what
  `artist_erasure.py --baseline uce --ckpt_name` and `generate_fid_images.py --erasure_ckpt_path` load - and
  info/erased-<name>.txt, the concepts as JSON.  --base enters the name only; anything but 2.1 raises.
"""
import argparse
import json
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import torch

from pdm.utils import uce as U
from pdm.utils.load_models import FrozenModels, cuda_device, inference_config


def parse_args(argv=None):
    return U.add_arguments(argparse.ArgumentParser(prog="TrainUSD")).parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    concepts, old_texts, new_texts, retain_texts, name = U.build_texts(
        args.concepts, args.concept_type, args.guided_concepts, args.preserve_concepts, args.preserve_number, args.add_prompts,
        args.technique, args.base, args.seed)
    preserve_scale = U.default_preserve_scale(args.preserve_scale, retain_texts)
    print(name)
    if args.ckpt_path is None:
        raise ValueError("--ckpt_path is required (the pruned checkpoint directory: arch_vector.pt + unet/)")
    config = inference_config(args.base_config_path, args.model_id, args.tiny, mixed_precision="no")
    models = FrozenModels(config, cuda_device(args.device))
    unet = models.load_unet(args.ckpt_path)
    U.edit_model(unet, models.text_encoder, models.tokenizer, old_texts, new_texts, retain_texts, lamb=U.LAMB,
                 erase_scale=args.erase_scale, preserve_scale=preserve_scale, technique=args.technique)
    out = os.path.join(args.output_dir, "models", f"erased-{name}.pt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    torch.save(unet.state_dict(), out)
    os.makedirs(os.path.join(args.output_dir, "info"), exist_ok=True)
    with open(os.path.join(args.output_dir, "info", f"erased-{name}.txt"), "w") as fp:
        json.dump(concepts, fp)
    print("Model saved at: ", out)
    return out


if __name__ == '__main__':
    main()
