#!/usr/bin/env python3
"""ConceptPrune, step 2 (the reference's baselines/concept_prune/save_union_over_time.py with its flags): the union over time
of the skilled weights as a mask on the pruned checkpoint, saved as the erasure checkpoint `artist_erasure.py --baseline
concept-prune --ckpt_name` and `generate_fid_images.py --erasure_ckpt_path` read.
    python scripts/baselines/concept_prune/save_union_over_time.py --target "Van Gogh" --base_config_path CFG \\
        --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/ --select_ratio 0.0

Reads skilled_neurons/<skill_ratio>/union_counts.pt of wanda.py, zeroes W where count > select_ratio * timesteps
(pdmk_wanda_apply on the fp32 weights), prints the share of masked weights per layer and writes
checkpoints/skill_ratio_<r>_timesteps_<T>_threshold<s>.pt: the full U-Net state dict under the reference's key names, the masked
layers' weights as fp16 (the kept values rounded through fp16, as the reference stores them).
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import torch

from pdm.utils import concept_prune as CP
from pdm.utils.load_models import FrozenModels, cuda_device, inference_config


def parse_args(argv=None):
    return CP.add_arguments(argparse.ArgumentParser()).parse_args(argv)


def main(argv=None):
    args = CP.resolve_args(parse_args(argv))
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    print("Arguments: ", args.__dict__)
    paths = CP.result_paths(args)
    counts_file = os.path.join(paths.skilled_neurons, "union_counts.pt")
    if not os.path.exists(counts_file):
        raise FileNotFoundError(f"{counts_file}: run wanda.py with the same flags first")
    counts = torch.load(counts_file, map_location="cpu")
    config = inference_config(args.base_config_path, args.model_id, args.tiny, args.mixed_precision)
    unet = FrozenModels(config, cuda_device(args.gpu)).load_unet(args.ckpt_path)
    print("Applying masks to the model")
    density = CP.apply_counts(unet, counts, args.select_ratio, args.timesteps)
    for l, (key, d) in enumerate(density.items()):
        print("Layer: ", l, key, "Density of skilled neurons: ", d)
    os.makedirs(paths.checkpoints, exist_ok=True)
    ckpt_name = os.path.join(paths.checkpoints, CP.checkpoint_name(args.skill_ratio, args.timesteps, args.select_ratio))
    torch.save(CP.masked_state_dict(unet), ckpt_name)
    print("Model saved at: ", ckpt_name)
    return ckpt_name


if __name__ == '__main__':
    main()
