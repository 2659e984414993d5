#!/usr/bin/env python3
"""ResNet-50 top-k classification of a folder of generated images, with the reference's name and flags
(baselines/unified-concept-editing/eval-scripts/imageclassify.py, the same file under baselines/erasing/oldcode_erasing_compvis):
    python scripts/baselines/unified_concept_editing/imageclassify.py --folder_path OUT/<edit> \\
        --prompts_path tests/golden/object_erasure/imagenette.csv [--save_path FILE.csv] [--topk 5] [--batch_size 250] \\
        [--resnet_weights resnet50-11ad3fa6.pth] [--categories_file imagenet_classes.txt]

* Every file of --folder_path whose name contains `.png` or `.jpg`, in sorted order, read as RGB, through torchvision's
  ImageClassification preset (Pillow bilinear resize of the short side to --resize_size, centre crop --crop_size, ImageNet
  normalisation) and pdm/models/resnet's ResNet-50 on the GPU; softmax and top-k are pdmk_softmax_topk (equal probabilities
  come lower index first).
* Output: the prompts frame inner-joined with the per-image results on `case_number` (the number before the first `_` of the
  file name), one row per image, plus `category_top{k}, index_top{k}, scores_top{k}` for k = 1 .. --topk.
* Weights: torchvision's resnet50-11ad3fa6.pth (IMAGENET1K_V2, `ResNet50_Weights.DEFAULT`) from --resnet_weights or torch
  hub's checkpoint cache; nothing is downloaded.
* Deviations from the reference: files are taken in sorted order, not os.listdir order; without --save_path the result goes
  to <folder>/<basename(folder)>_classification.csv (the reference's default raises NameError); without --categories_file
  (1000 lines, one name each - torchvision's `weights.meta["categories"]`, which is not shipped here) `category_top{k}` holds
  the Imagenette name where the index is one of the ten classes and the index as text otherwise.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from pdm.utils import object_erasure as O


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='ImageClassification',
                                     description='Takes the path of images and generates classification scores')
    parser.add_argument('--folder_path', help='path to images', type=str, required=True)
    parser.add_argument('--prompts_path', help='path to prompts', type=str, required=True)
    parser.add_argument('--save_path', help='path to save results', type=str, required=False, default=None)
    parser.add_argument('--device', type=str, required=False, default='cuda:0')
    parser.add_argument('--topk', type=int, required=False, default=5)
    parser.add_argument('--batch_size', type=int, required=False, default=250)
    # --- additions of this build
    parser.add_argument('--resnet_weights', type=str, default=None, help="torchvision's resnet50-11ad3fa6.pth")
    parser.add_argument('--categories_file', type=str, default=None, help="1000 ImageNet category names, one per line")
    parser.add_argument('--resize_size', type=int, default=232)
    parser.add_argument('--crop_size', type=int, default=224)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    categories = O.load_categories(args.categories_file) if args.categories_file else None
    save_path = args.save_path if args.save_path is not None else O.default_save_path(args.folder_path)
    from pdm.models.resnet import ResNet50Classifier
    model = ResNet50Classifier.from_pretrained(args.resnet_weights, device=args.device)
    O.classify_folder(args.folder_path, args.prompts_path, save_path, model, topk=args.topk, batch_size=args.batch_size,
                      categories=categories, resize_size=args.resize_size, crop_size=args.crop_size)
    return save_path


if __name__ == '__main__':
    main()
