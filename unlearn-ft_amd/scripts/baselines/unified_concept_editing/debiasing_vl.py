#!/usr/bin/env python3
"""Debias-VL at sampling time, with the reference's flags (baselines/unified-concept-editing/eval-scripts/debiasing_vl.py):
    python scripts/baselines/unified_concept_editing/debiasing_vl.py --model_name original \\
        --prompts_path PROMPTS.csv --save_path OUT [--debias_concepts "Doctor,Nurse"] --base_config_path CFG \\
        --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/ [--mixed_precision bf16]

A calibration matrix P = inv(500 M + I), built once per run from the `male` / `female` prompt pairs of --debias_concepts (empty:
the list of configs/baselines/debias_vl.yaml), multiplies the conditional prompt embeddings; the unconditional ones stay
(pdm/utils/debias_vl.py).  The system is formed, factored and solved in fp64 on the GPU and no inverse is formed.
It changes no weights, so --model_name may be `original` (the pruned checkpoint --ckpt_path itself) or any erasure checkpoint,
laid over it as generate_images.py does.

* Rows, seeds, batch and output as generate_images.py: <save_path>/<model_name without "diffusers-" and ".pt">/
  <case_number>_<n>.png, which CLIP_classify.py reads.  The prompt is encoded once per row, its 77 rows are transformed in
  fp32 and repeated over the --num_samples batch.
* --scheduler lms samples as the reference does, with K-LMS (LMSDiscreteScheduler): --ddim_steps then counts LMS
  steps and the initial noise is scaled by the largest sigma.
* Deviations from the reference: the default --scheduler pndm is the project's captured PNDM sampler, and --ddim_steps counts
  PNDM steps there; the LMS scheduler is a restatement (diffusers is not available to pin it against, and no real SD-2.1
  weights were sampled with it) with exact coefficient integrals; the models are the pruned SD-2.1 student
  and its text encoder loaded through FrozenModels, not SD-1.4 / CLIP-L from the hub, so --base is not offered.
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import torch

from pdm.utils import concept_algebra as A
from pdm.utils import debias_vl as D
from pdm.utils import sld as S


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='generateImages', description='Generate Images using Diffusers Code', allow_abbrev=False)
    A.add_common_arguments(parser)
    parser.add_argument('--debias_concepts', help='Concepts to debias', type=str, required=False, default='')
    return parser.parse_args(argv)


@torch.no_grad()
def generate_images(pipe, factor, model_name, prompts_path, save_path, guidance_scale=7.5, image_size=512, ddim_steps=100,
                    num_samples=10, from_case=0, till_case=1000000):
    uncond = pipe.text_encoder(pipe._tokenize([""]))[0]

    def prompt_kwargs(prompt, n):
        text = D.apply(factor, pipe.text_encoder(pipe._tokenize([prompt]))[0])
        return dict(prompt_embeds=text.expand(n, -1, -1), negative_prompt_embeds=uncond.expand(n, -1, -1))

    return S.sample_cases(pipe, prompts_path, A.folder_path(save_path, model_name), from_case=from_case, till_case=till_case,
                          num_samples=num_samples, prompt_kwargs=prompt_kwargs, guidance_scale=guidance_scale, height=image_size,
                          width=image_size, num_inference_steps=ddim_steps)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    concepts = D.split_concepts(args.debias_concepts)
    models, pipe = A.load_pipeline(args)
    factor = D.calibration(models, concepts)
    return generate_images(pipe, factor, args.model_name, args.prompts_path, args.save_path,
                           guidance_scale=args.guidance_scale, image_size=args.image_size, ddim_steps=args.ddim_steps,
                           num_samples=args.num_samples, from_case=args.from_case, till_case=args.till_case)


if __name__ == '__main__':
    main()
