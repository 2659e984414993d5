"""Text features of the CLIP score (the reference's scripts/metrics/clip_features.py, same flags): one normalised fp32 [D]
`.npy` per caption file of --dataset_path, written to <dirname(dataset_path)>/<model tag>_clip_features/.
--tokenizer: a local CLIPTokenizer directory (an OpenAI .pt has no vocabulary); --dtype: the encoders' compute dtype."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from pdm.utils.clip_utils import clip_features

logging.basicConfig(level=logging.INFO)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--dataset_path', type=str, required=True)
    parser.add_argument('--clip_model', type=str, default="ViT-B/32")
    parser.add_argument('--num_workers', type=int, default=None)
    parser.add_argument('--batch_size', type=int, default=64)
    parser.add_argument('--tokenizer', type=str, default=None,
                        help="local CLIPTokenizer directory (default: the --clip_model directory)")
    parser.add_argument('--dtype', type=str, default="fp32", choices=sorted(DTYPES))
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    return clip_features(args.dataset_path, clip_model=args.clip_model, num_workers=args.num_workers,
                         batch_size=args.batch_size, tokenizer=args.tokenizer, dtype=DTYPES[args.dtype])


if __name__ == '__main__':
    main()
