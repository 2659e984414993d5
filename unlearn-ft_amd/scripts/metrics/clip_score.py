"""CLIP score of generated images (the reference's scripts/metrics/clip_score.py, same flags): appends
"{gen_images_dir} {score}" to {result_dir}/clip_score_{dataset_name}.txt.  Images and text features pair by file stem.
--tokenizer is accepted for symmetry with clip_features.py (the text features are precomputed); --dtype: compute dtype."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from pdm.utils.clip_utils import clip_score

logging.basicConfig(level=logging.INFO)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--gen_images_dir', type=str, required=True)
    parser.add_argument('--text_features_dir', type=str, required=True)
    parser.add_argument('--clip_model', type=str, default="ViT-B/32")
    parser.add_argument('--num_workers', type=int, default=None)
    parser.add_argument('--batch_size', type=int, default=64)
    parser.add_argument('--result_dir', type=str, required=True, help="Directory to save the results")
    parser.add_argument('--dataset_name', type=str, required=True, help="Dataset name")
    parser.add_argument('--tokenizer', type=str, default=None, help="unused: the text features are precomputed")
    parser.add_argument('--dtype', type=str, default="fp32", choices=sorted(DTYPES))
    return parser.parse_args(argv)


def result_file(result_dir, dataset_name):
    return f"{result_dir}/clip_score_{dataset_name}.txt"


def write_result(result_dir, dataset_name, gen_images_dir, score):
    os.makedirs(result_dir, exist_ok=True)
    with open(result_file(result_dir, dataset_name), "a") as f:
        f.write(f"{gen_images_dir} {score}\n")


def main(argv=None):
    args = parse_args(argv)
    logging.info(f"Calculating CLIP score for {args.gen_images_dir} using {args.text_features_dir} as text features.")
    score = clip_score(args.text_features_dir, args.gen_images_dir, clip_model=args.clip_model, num_workers=args.num_workers,
                       batch_size=args.batch_size, dtype=DTYPES[args.dtype])
    logging.info(f"CLIP score: {score}")
    write_result(args.result_dir, args.dataset_name, args.gen_images_dir, score)
    return score


if __name__ == '__main__':
    main()
