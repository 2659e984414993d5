#!/usr/bin/env python3
"""ConceptPrune, step 1 (the reference's baselines/concept_prune/wanda.py with its flags): observe the feed-forward activations
of the pruned checkpoint for base and concept prompts and count, per weight of every `...ff.net.2`, the timesteps at which it
is "skilled" for the concept.
    python scripts/baselines/concept_prune/wanda.py --target "Van Gogh" --base_config_path CFG \\
        --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/ [--mixed_precision bf16]

* Settings: configs/baselines/concept_prune_wanda.yaml (the reference's wanda_config.yaml values); flags replace them.
* Prompts (pdm/utils/concept_prune.py build_prompts): art targets `a photo of a {thing}` / `a {thing} in the style of {target}`
  over tests/golden/concept_prune/things.txt, `naked` over humans.txt.  Object, gender and memorize targets raise.
* Observation: per pair one image from each prompt with the same seed, --timesteps steps (50), guidance 7.5, DDIM (one U-Net
  call per step; --scheduler pndm adds its repeated first call to slot 0), at sample_size x 8 of <model_id>/unet/config.json.
  The engine hands every GEGLU output to a WandaObserver (pdmk_rownorm_colsq): nothing leaves the device while sampling.
  base_norms.pt / target_norms.pt ({t: {l: tensor[F]}}, the reference's format) are written to the result directory and
  reloaded from there when present; the first five image pairs go to images/.  --dbg stops after three pairs.
* Scores: pdmk_wanda_count per layer, all timesteps in one launch; skilled_neurons/<skill_ratio>/union_counts.pt holds
  {layer key: int32 [O, F]}.  The reference's per-timestep pickles are not written.
* Result path: <--result_dir or results/results_seed_<seed>/<res_path.split('/')[1]>>/<model>/<target>/.
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import torch

from pdm.utils import concept_prune as CP
from pdm.utils import erasure_utils as E
from pdm.utils.load_models import FrozenModels, cuda_device, inference_config


def parse_args(argv=None):
    return CP.add_arguments(argparse.ArgumentParser()).parse_args(argv)


def main(argv=None):
    args = CP.resolve_args(parse_args(argv))
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    print("Arguments: ", args.__dict__)
    paths = CP.result_paths(args)
    base_prompts, target_prompts = CP.build_prompts(args.target, args.base, args.words_dir)
    if args.dbg:
        base_prompts, target_prompts = base_prompts[:3], target_prompts[:3]
    for d in (paths.images, paths.skilled_neurons, paths.checkpoints):
        os.makedirs(d, exist_ok=True)
    device = cuda_device(args.gpu)
    models = FrozenModels(inference_config(args.base_config_path, args.model_id, args.tiny, args.mixed_precision), device)
    pipe = models.pipeline(models.load_unet(args.ckpt_path), args.scheduler)
    unet = pipe.unet
    layers = CP.ffn_layers(unet)
    print("Layer names: ", [key for key, *_ in layers], len(layers))

    base_file, target_file = (os.path.join(paths.res_path, n) for n in ("base_norms.pt", "target_norms.pt"))
    if not (os.path.exists(base_file) and os.path.exists(target_file)):
        obs = [CP.WandaObserver(unet, args.timesteps, repeat_first=args.scheduler == "pndm") for _ in range(2)]
        CP.observe(pipe, obs[0], obs[1], base_prompts, target_prompts, args.seed, args.timesteps,
                   E.image_resolution(args.model_id, args.image_resolution), paths.images)
        obs[0].save(base_file)
        obs[1].save(target_file)
        print("Saved norms in: ", base_file)
    base_norms, target_norms = CP.load_norms(base_file, device), CP.load_norms(target_file, device)
    if len(base_norms[0]) != args.timesteps:
        raise ValueError(f"{base_file}: {len(base_norms[0])} timesteps, --timesteps {args.timesteps}")

    counts = CP.union_counts(unet, base_norms, target_norms, args.skill_ratio)
    out = os.path.join(paths.skilled_neurons, "union_counts.pt")
    torch.save(counts, out)
    print("Saved counts in: ", out)
    return out


if __name__ == '__main__':
    main()
