#!/usr/bin/env python3
"""CLIP zero-shot attribute shares of a folder of generated images (the reference's baselines/unified-concept-editing/
eval-scripts/CLIP_classify.py with its flags): per case of the prompts CSV, the share of its images that CLIP puts closest to
each attribute text.
    python scripts/baselines/unified_concept_editing/CLIP_classify.py --im_path <images> --prompts_path <prompts.csv> \\
        --attributes "a man,a woman" --clip_model <clip-vit-base-patch32 directory or ViT-B-32.pt>

* Files: names containing `.png`, natural-sorted, `<case>_<n>.png`, kept when --from_case <= case <= --till_case; a file that
  cannot be decoded counts as a row of zeros (the reference's `except`).
* Per image: CLIPProcessor's transform (pdmk_image_prep_ex, bicubic) and the image tower, then pdmk_zeroshot_head against the
  attribute texts: mask = the logits that equal the row's largest, added to a per-case table on the device; one read-back.
* Writes <--save_path>/<folder>_gender_classify.csv (default: beside the folder): the prompts frame plus one `<attribute>_bias`
  column per attribute (spaces written as `_`) with the mean mask of the case's images, joined on `case_number` as
  imageclassify.py's frame is (pdm/utils/object_erasure.py merge_on_case_number); no index column.
* --clip_model is resolved like clip_score.py's: a local transformers directory or an OpenAI .pt; a hub id raises.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import torch

from pdm.utils import uce_debias as D


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog="CLIP classification",
                                     description="Takes the path to images and gives CLIP classification scores")
    parser.add_argument("--im_path", help="path to images", type=str, required=True)
    parser.add_argument("--attributes", help="comma separated attributes to classify against", type=str, default="a man,a woman")
    parser.add_argument("--prompts_path", help="path to csv prompts", type=str, required=True)
    parser.add_argument("--save_path", help="path to save results", type=str, default=None)
    parser.add_argument("--from_case", help="case number start", type=int, default=0)
    parser.add_argument("--till_case", help="case number end", type=int, default=1000000000)
    # --- additions of this build
    parser.add_argument("--clip_model", type=str, default="openai/clip-vit-base-patch32")
    parser.add_argument("--tokenizer", type=str, default=None, help="CLIP tokenizer directory (default: --clip_model's)")
    parser.add_argument("--device", type=str, default="0")
    parser.add_argument("--batch_size", type=int, default=64)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from pdm.models.clip import convert
    from pdm.models.clip.clip_model import CLIPModel
    from pdm.utils.clip_utils import _tokenizer_for
    from pdm.utils.load_models import cuda_device
    convert.resolve(args.clip_model)                      # a hub id raises here, before any model is built
    attributes = [a.strip() for a in args.attributes.split(",")]
    device = cuda_device(args.device)
    clip = CLIPModel.from_pretrained(args.clip_model, dtype=torch.float32, device=device)
    tokenizer = _tokenizer_for(args.clip_model, args.tokenizer)
    path, _header, _rows = D.classify_folder(clip, tokenizer, args.im_path, attributes, args.prompts_path, args.save_path,
                                             args.from_case, args.till_case, args.batch_size)
    return path


if __name__ == '__main__':
    main()
