#!/usr/bin/env python3
"""Safe Latent Diffusion images with the reference's name and flags (baselines/unified-concept-editing/eval-scripts/
sld-generate-images.py, the same file under baselines/erasing): the inference-time erasure baseline - no weight changes, a
third "safety concept" branch in classifier-free guidance (pdm/pipelines/pruning_pipelines.py, pdmk_sld_*).
    python scripts/baselines/unified_concept_editing/sld_generate_images.py --sld_concept "Van Gogh" --sld_type Medium \\
        --prompts_path tests/golden/artist_prompts/test_Van\\ Gogh.csv --save_path OUT --base_config_path CFG \\
        --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/ [--erasure_ckpt_path FILE] [--mixed_precision bf16]

* Rows: `case_number, prompt, evaluation_seed` of --prompts_path in file order, from --from_case on.
* Per row: `torch.Generator(device).manual_seed(evaluation_seed)`, --num_samples images of the prompt as one batch, PNDM with
  --ddim_steps steps at --image_size, guidance --guidance_scale, the preset --sld_type (Weak / Medium / Strong / Max of
  configs/baselines/sld.yaml; anything else raises) against --sld_concept (none: the default safety sentence of that file).
  uint8 as diffusers' numpy_to_pil (rounded), PNG.
* Output: <save_path>/SLD_<sld_type>_<sld_concept>/<case_number>_<n>.png, the reference's names.
* Deviations from the reference: its leftover filter that keeps only the cases 0, 38 and 51 is not reproduced; the models are
  the pruned checkpoint --ckpt_path (optionally with an erasure checkpoint laid over it) loaded through FrozenModels, not
  SD-1.4 from the hub; --ddim_steps reaches the sampler (the reference parses it and samples with the pipeline's default 50);
  the default --scheduler pndm is the project's captured PNDM sampler.  --scheduler lms samples with K-LMS
  (LMSDiscreteScheduler as the sibling evaluation scripts configure it): --ddim_steps then counts LMS steps, the
  warm-up counts LMS's U-Net calls (one per step), and the scheduler is a restatement that diffusers was not available to pin.
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
    parser = argparse.ArgumentParser(prog='generateImages', description='Generate Images with Safe Latent Diffusion')
    parser.add_argument('--sld_concept', help='concept to remove from SLD', type=str, required=False, default=None)
    parser.add_argument('--prompts_path', help='path to csv file with prompts', type=str, required=True)
    parser.add_argument('--save_path', help='folder where to save images', type=str, required=True)
    parser.add_argument('--device', help='cuda device to run on', type=str, required=False, default='cuda:0')
    parser.add_argument('--guidance_scale', help='guidance to run eval', type=float, required=False, default=7.5)
    parser.add_argument('--image_size', help='image size used to train', type=int, required=False, default=512)
    parser.add_argument('--from_case', help='continue generating from case_number', type=int, required=False, default=0)
    parser.add_argument('--num_samples', help='number of samples per prompt', type=int, required=False, default=1)
    parser.add_argument('--ddim_steps', help='ddim steps of inference used to train', type=int, required=False, default=50)
    parser.add_argument('--sld_type', help='Type of SLD', type=str, required=False, default='Medium')
    # --- local model loading, as the other baseline scripts
    parser.add_argument('--base_config_path', type=str, default=None)
    parser.add_argument('--model_id', type=str, default='stabilityai/stable-diffusion-2-1')
    parser.add_argument('--ckpt_path', type=str, default=None, help="the pruned checkpoint directory: arch_vector.pt + unet/")
    parser.add_argument('--erasure_ckpt_path', type=str, default=None, help="an ESD / UCE / ConceptPrune checkpoint laid over it")
    parser.add_argument('--mixed_precision', type=str, default=None, choices=["no", "bf16"])
    parser.add_argument('--tiny', action="store_true", help="tiny U-Net topology (tests)")
    parser.add_argument('--scheduler', type=str, default='pndm', choices=["pndm", "lms"],
                        help="sampler: the project's PNDM (default) or K-LMS (LMSDiscreteScheduler)")
    return parser.parse_args(argv)


@torch.no_grad()
def generate_SLD(pipe, sld_concept, sld_type, prompts_path, save_path, guidance_scale=7.5, image_size=512, ddim_steps=50,
                 num_samples=1, from_case=0):
    kw = S.sampling_kwargs(sld_type, sld_concept)
    print(kw["safety_concept"])
    return S.sample_cases(pipe, prompts_path, S.folder_path(save_path, sld_type, sld_concept), from_case=from_case,
                          num_samples=num_samples, guidance_scale=guidance_scale, height=image_size, width=image_size,
                          num_inference_steps=ddim_steps, **kw)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    S.preset(args.sld_type)                               # an unknown type raises before anything is loaded
    if args.ckpt_path is None:
        raise ValueError("--ckpt_path is required (the pruned checkpoint directory: arch_vector.pt + unet/)")
    device = torch.device(args.device)
    if device.type != "cuda":
        raise ValueError(f"--device {args.device}: the samplers run on the GPU only")
    config = inference_config(args.base_config_path, args.model_id, args.tiny, args.mixed_precision)
    models = FrozenModels(config, cuda_device(device.index or 0))
    unet = models.load_unet(args.ckpt_path)
    if args.erasure_ckpt_path is not None:
        from pdm.utils.erasure_utils import load_erasure_checkpoint
        load_erasure_checkpoint(unet, args.erasure_ckpt_path)
    return generate_SLD(models.pipeline(unet, kind=args.scheduler), args.sld_concept, args.sld_type, args.prompts_path, args.save_path,
                        guidance_scale=args.guidance_scale, image_size=args.image_size, ddim_steps=args.ddim_steps,
                        num_samples=args.num_samples, from_case=args.from_case)


if __name__ == '__main__':
    main()
