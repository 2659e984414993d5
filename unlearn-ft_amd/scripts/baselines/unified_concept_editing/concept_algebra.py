#!/usr/bin/env python3
"""Concept-algebra debiasing at sampling time, with the reference's flags
(baselines/unified-concept-editing/eval-scripts/concept_algebra.py):
    python scripts/baselines/unified_concept_editing/concept_algebra.py --model_name original \\
        --prompts_path PROMPTS.csv --save_path OUT [--concepts_to_project "a man,a woman,a person"] --base_config_path CFG \\
        --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/ [--mixed_precision bf16]

Five U-Net branches per step - uncond, text and the three concepts p0, p1, p2 - and the text score loses its component along
p1 - p0, measured against p2, over the whole batch (include/pdmk.h "Concept algebra").  It changes no weights, so
--model_name may be `original` (the pruned checkpoint --ckpt_path itself) or any erasure checkpoint (ESD / UCE / ConceptPrune /
`unbiased-*.pt`), laid over it as generate_images.py does.

* Rows, seeds, batch and output as generate_images.py: <save_path>/<model_name without "diffusers-" and ".pt">/
  <case_number>_<n>.png, which CLIP_classify.py reads.
* --concepts_to_project: exactly three, comma separated; anything else raises.
* --scheduler lms samples as the reference does, with K-LMS (LMSDiscreteScheduler): --ddim_steps then counts LMS
  steps and the initial noise is scaled by the largest sigma.
* Deviations from the reference: the default --scheduler pndm is the project's captured PNDM sampler, and --ddim_steps counts
  PNDM steps there; the LMS scheduler is a restatement (diffusers is not available to pin it against, and no real SD-2.1
  weights were sampled with it) with exact coefficient integrals; the models are the pruned SD-2.1 student
  loaded through FrozenModels, not SD-1.4 / CLIP-L from the hub, so --base is not offered; where the direction p1 - p0 is zero
  the projection is left out (the reference divides by zero and samples NaN).
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import torch

from pdm.utils import concept_algebra as A
from pdm.utils import sld as S


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='generateImages', description='Generate Images using Diffusers Code', allow_abbrev=False)
    A.add_common_arguments(parser)
    parser.add_argument('--concepts_to_project', help='concepts to project', type=str, required=False, default=A.DEFAULT_CONCEPTS)
    return parser.parse_args(argv)


@torch.no_grad()
def generate_images(pipe, model_name, prompts_path, concepts_to_project, save_path, guidance_scale=7.5, image_size=512,
                    ddim_steps=100, num_samples=10, from_case=0, till_case=1000000):
    if len(concepts_to_project) != 3:
        raise ValueError("Must provide 3 concepts to project")
    embeds = pipe.text_encoder(pipe._tokenize(list(concepts_to_project)))[0]          # each concept encoded once per run
    return S.sample_cases(pipe, prompts_path, A.folder_path(save_path, model_name), from_case=from_case, till_case=till_case,
                          num_samples=num_samples, guidance_scale=guidance_scale, height=image_size, width=image_size,
                          num_inference_steps=ddim_steps, algebra_embeds=embeds)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    concepts = A.split_concepts(args.concepts_to_project)
    _, pipe = A.load_pipeline(args)
    return generate_images(pipe, args.model_name, args.prompts_path, concepts, args.save_path,
                           guidance_scale=args.guidance_scale, image_size=args.image_size, ddim_steps=args.ddim_steps,
                           num_samples=args.num_samples, from_case=args.from_case, till_case=args.till_case)


if __name__ == '__main__':
    main()
