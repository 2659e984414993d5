#!/usr/bin/env python3
"""ConceptPrune, the method itself (the reference's baselines/concept_prune/remove_neurons.py with its flags): sample the target
prompts with the skilled neurons of every timestep removed - at U-Net call t, layer l's `ff.net.2` runs with
W * (1 - mask[t][l]) - next to the same prompts sampled plainly, and save the pairs side by side.
    python scripts/baselines/concept_prune/remove_neurons.py --target "Van Gogh" --base_config_path CFG \\
        --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/ [--mixed_precision bf16]

* Settings, flags, prompts and the result path are wanda.py's (configs/baselines/concept_prune_wanda.yaml; pdm/utils/
  concept_prune.py).  --target_file is the reference's flag for its memorize targets, which are not built: passing it raises.
* Input: base_norms.pt / target_norms.pt of wanda.py in the result directory (FileNotFoundError without them, before a GPU is
  touched).  The masks are formed from them on the device (TimestepMasks.from_norms: pdmk_wanda_select per layer, one bit per
  timestep and weight); the reference's per-timestep pickles are neither read nor written.
* Per target prompt (--dbg: the first two): one image sampled plainly and one with `neuron_masks=` from the same seed, with
  wanda.py's steps, guidance 7.5, scheduler and resolution (DDIM: the captured loop, pdmk_masked_weights as its first node).
  Both are resized to 256 x 256 and pasted at (0, 40) and (275, 40) of a 530 x 290 canvas, the prompt written at (80, 15) and
  `w/o skilled neurons` at (350, 15): <res>/after_removal_results/<skill_ratio>/img_{i}_{prompt}.jpg.
* mask_density.json in that folder: {layer key: [share of masked weights at each timestep]}.  Returns the folder.
* Deviation: the reference re-seeds the global generators (torch.manual_seed) before each of the two images; here each image
  takes a device generator seeded with --seed, as wanda.py's observation does.
"""
import argparse
import json
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import torch

from pdm.utils import concept_prune as CP
from pdm.utils import erasure_utils as E
from pdm.utils.load_models import FrozenModels, cuda_device, inference_config

CANVAS, TILE, LEFT, RIGHT = (530, 290), (256, 256), (0, 40), (275, 40)
PROMPT_AT, LABEL_AT, LABEL = (80, 15), (350, 15), "w/o skilled neurons"


def parse_args(argv=None):
    parser = CP.add_arguments(argparse.ArgumentParser())
    parser.add_argument("--target_file", type=str, default=None)
    return parser.parse_args(argv)


def compose(plain, removed, prompt):
    """The reference's canvas: the two images (uint8 HWC arrays) side by side under their captions."""
    from PIL import Image, ImageDraw
    canvas = Image.new("RGB", CANVAS)
    canvas.paste(Image.fromarray(plain).resize(TILE), LEFT)
    canvas.paste(Image.fromarray(removed).resize(TILE), RIGHT)
    draw = ImageDraw.Draw(canvas)
    draw.text(PROMPT_AT, prompt, (255, 255, 255))
    draw.text(LABEL_AT, LABEL, (255, 255, 255))
    return canvas


@torch.no_grad()
def remove_skilled_neurons(pipe, masks, prompts, seed, steps, resolution, save_path):
    for i, prompt in enumerate(prompts):
        print("text: ", prompt)
        images = []
        for neuron_masks in (None, masks):
            gen = torch.Generator(device=pipe.device).manual_seed(int(seed))
            images.append(pipe(prompt=[prompt], num_inference_steps=steps, guidance_scale=CP.GUIDANCE, generator=gen,
                               height=resolution, width=resolution, output_type="u8_round", neuron_masks=neuron_masks).images[0])
        name = os.path.join(save_path, f"img_{i}_{prompt}.jpg")
        print("Saving image in: ", name)
        compose(images[0], images[1], prompt).save(name)


def main(argv=None):
    args = CP.resolve_args(parse_args(argv))
    if args.target_file is not None:
        raise NotImplementedError("--target_file: read by the memorize targets only, which are not built here")
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    print("Arguments: ", args.__dict__)
    paths = CP.result_paths(args)
    base_file, target_file = (os.path.join(paths.res_path, n) for n in ("base_norms.pt", "target_norms.pt"))
    for f in (base_file, target_file):
        if not os.path.exists(f):
            raise FileNotFoundError(f"{f}: run wanda.py with the same flags first")
    _base_prompts, target_prompts = CP.build_prompts(args.target, args.base, args.words_dir)
    if args.dbg:
        target_prompts = target_prompts[:2]
    device = cuda_device(args.gpu)
    models = FrozenModels(inference_config(args.base_config_path, args.model_id, args.tiny, args.mixed_precision), device)
    pipe = models.pipeline(models.load_unet(args.ckpt_path), args.scheduler)
    base_norms, target_norms = CP.load_norms(base_file, device), CP.load_norms(target_file, device)
    if len(base_norms[0]) != args.timesteps:
        raise ValueError(f"{base_file}: {len(base_norms[0])} timesteps, --timesteps {args.timesteps}")
    masks = CP.TimestepMasks.from_norms(pipe.unet, base_norms, target_norms, args.skill_ratio)
    os.makedirs(paths.after_removal_results, exist_ok=True)
    with open(os.path.join(paths.after_removal_results, "mask_density.json"), "w") as f:
        json.dump(masks.density(), f)
    remove_skilled_neurons(pipe, masks, target_prompts, args.seed, args.timesteps,
                           E.image_resolution(args.model_id, args.image_resolution), paths.after_removal_results)
    return paths.after_removal_results


if __name__ == '__main__':
    main()
