#!/usr/bin/env python3
"""Images of the original or of an edited model for the evaluation scripts, with the reference's flags
(baselines/unified-concept-editing/eval-scripts/generate-images.py, the same file under baselines/erasing):
    python scripts/baselines/unified_concept_editing/generate_images.py --model_name original \\
        --prompts_path tests/golden/artist_prompts/test_Van\\ Gogh.csv --save_path OUT --base_config_path CFG \\
        --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/ [--mixed_precision bf16]

* --model_name original samples the pruned checkpoint --ckpt_path itself; anything else is an erasure checkpoint (ESD / UCE /
  ConceptPrune) laid over it with load_erasure_checkpoint: the file --model_name if it exists, else <--models_dir>/<model_name>
  (the reference's `models/<model_name>`).
* Rows: `case_number, prompt, evaluation_seed` of --prompts_path with --from_case <= case_number <= --till_case, in file order.
  Per row `torch.Generator(device).manual_seed(evaluation_seed)` and --num_samples images of the prompt as one batch.
* Output: <save_path>/<model_name without "diffusers-" and ".pt">/<case_number>_<n>.png - the layout lpips_eval.py and
  styleloss.py read (run it once with `original` and once per edit, same prompts, same seeds).
* --scheduler lms samples as the reference does, with K-LMS (LMSDiscreteScheduler, scaled_linear 0.00085 ... 0.012, 1000 train
  steps): --ddim_steps then counts LMS steps and the initial noise is scaled by the largest sigma.
* Deviations from the reference: the default --scheduler pndm is the project's captured PNDM sampler, and --ddim_steps counts
  PNDM steps there; the LMS scheduler is a restatement (diffusers is not available to pin it against, and no real SD-2.1
  weights were sampled with it) with exact coefficient integrals; the models are the pruned checkpoint loaded
  through FrozenModels, not SD-1.x from the hub, so --base is not offered; the row loop is the one of sld_generate_images.py
  (pdm/utils/sld.py sample_cases).
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import torch

from pdm.utils import sld as S
from pdm.utils.load_models import FrozenModels, cuda_device, inference_config


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='generateImages', description='Generate Images using Diffusers Code')
    parser.add_argument('--model_name', help='name of model', type=str, required=True)
    parser.add_argument('--prompts_path', help='path to csv file with prompts', type=str, required=True)
    parser.add_argument('--save_path', help='folder where to save images', type=str, required=True)
    parser.add_argument('--device', help='cuda device to run on', type=str, required=False, default='cuda:0')
    parser.add_argument('--guidance_scale', help='guidance to run eval', type=float, required=False, default=7.5)
    parser.add_argument('--image_size', help='image size used to train', type=int, required=False, default=512)
    parser.add_argument('--till_case', help='continue generating from case_number', type=int, required=False, default=1000000)
    parser.add_argument('--from_case', help='continue generating from case_number', type=int, required=False, default=0)
    parser.add_argument('--num_samples', help='number of samples per prompt', type=int, required=False, default=1)
    parser.add_argument('--ddim_steps', help='ddim steps of inference used to train', type=int, required=False, default=100)
    # --- local model loading, as the other baseline scripts
    parser.add_argument('--models_dir', type=str, default='models', help="where --model_name is looked up when it is not a file")
    parser.add_argument('--base_config_path', type=str, default=None)
    parser.add_argument('--model_id', type=str, default='stabilityai/stable-diffusion-2-1')
    parser.add_argument('--ckpt_path', type=str, default=None, help="the pruned checkpoint directory: arch_vector.pt + unet/")
    parser.add_argument('--mixed_precision', type=str, default=None, choices=["no", "bf16"])
    parser.add_argument('--tiny', action="store_true", help="tiny U-Net topology (tests)")
    parser.add_argument('--scheduler', type=str, default='pndm', choices=["pndm", "lms"],
                        help="sampler: the project's PNDM (default) or the reference's K-LMS (LMSDiscreteScheduler)")
    return parser.parse_args(argv)


def folder_path(save_path, model_name):
    """generate-images.py:42, of the last path component when --model_name is a file path."""
    name = os.path.basename(model_name.rstrip("/")) or model_name
    return f'{save_path}/{name.replace("diffusers-", "").replace(".pt", "")}'


def erasure_checkpoint(model_name, models_dir):
    """None for `original`; else the file to lay over the pruned checkpoint (FileNotFoundError naming both places tried)."""
    if model_name == 'original':
        return None
    for path in (model_name, os.path.join(models_dir, model_name)):
        if os.path.exists(path):
            return path
    raise FileNotFoundError(f"--model_name {model_name}: neither {model_name} nor {os.path.join(models_dir, model_name)} exists")


@torch.no_grad()
def generate_images(pipe, model_name, prompts_path, save_path, guidance_scale=7.5, image_size=512, ddim_steps=100, num_samples=10,
                    from_case=0, till_case=1000000):
    return S.sample_cases(pipe, prompts_path, folder_path(save_path, model_name), from_case=from_case, till_case=till_case,
                          num_samples=num_samples, guidance_scale=guidance_scale, height=image_size, width=image_size,
                          num_inference_steps=ddim_steps)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    if args.ckpt_path is None:
        raise ValueError("--ckpt_path is required (the pruned checkpoint directory: arch_vector.pt + unet/)")
    device = torch.device(args.device)
    if device.type != "cuda":
        raise ValueError(f"--device {args.device}: the samplers run on the GPU only")
    erasure = erasure_checkpoint(args.model_name, args.models_dir)
    config = inference_config(args.base_config_path, args.model_id, args.tiny, args.mixed_precision)
    models = FrozenModels(config, cuda_device(device.index or 0))
    unet = models.load_unet(args.ckpt_path)
    if erasure is not None:
        from pdm.utils.erasure_utils import load_erasure_checkpoint
        load_erasure_checkpoint(unet, erasure)
    return generate_images(models.pipeline(unet, kind=args.scheduler), args.model_name, args.prompts_path, args.save_path,
                           guidance_scale=args.guidance_scale, image_size=args.image_size, ddim_steps=args.ddim_steps,
                           num_samples=args.num_samples, from_case=args.from_case, till_case=args.till_case)


if __name__ == '__main__':
    main()
