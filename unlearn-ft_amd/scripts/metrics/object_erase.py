#!/usr/bin/env python3
"""Object-erasure accuracy on Imagenette with the reference's name and flags
(baselines/concept_prune/benchmarking/object_erase.py): is the erased class gone, and are the other nine still there?
    python scripts/metrics/object_erase.py --target "church" --removal_mode erase --baseline pdm --base_config_path CFG \\
        --model_id <SD-2.1 snapshot> --original_ckpt <pruned>/checkpoint-N/ --ckpt_name <erased>/checkpoint-M/ \\
        [--resnet_weights resnet50-11ad3fa6.pth] [--mixed_precision bf16]

* Rows: --prompts_csv (default tests/golden/object_erasure/imagenette.csv, the reference's datasets/imagenette.csv: 5000
  prompts `an image of a <class>`, 500 per class).  `erase`: the rows whose `class` (or `label_str`) equals --target,
  case-insensitive; `keep`: all others, each with its own label.  --dbg stops after 11 rows.
* Generation, only while the image directory is empty: row i is sampled from `torch.Generator(device).manual_seed(
  evaluation_seed)` with the model --baseline selects (artist_erasure.py's loader and baselines), 50 steps, guidance 7.5, at
  sample_size x 8 of <model_id>/unet/config.json, and written as `removed_{i}.png`.  --sld_type samples with Safe Latent
  Diffusion, as artist_erasure.py.
* Scoring, always, from the files: ResNet-50 (pdm/models/resnet; --resnet_weights or torch hub's cache, never downloaded),
  torchvision's preset (--resize_size 232, --crop_size 224), top-1 by pdmk_softmax_topk; a hit when the predicted index is
  the label's ImageNet index (configs/baselines/imagenette.yaml).  `{"average_accuracy": hits / rows}` goes to
  <images>/results_<mode>_<p>.json, p = ckpt_name.split('/')[-1].split('.pt')[0] or `concept-prune`, as the reference.
* Result path: <--result_dir or results/results_seed_<seed>/<res_path.split('/')[2]>>/<model>/<target>/<baseline>/
  benchmarking/concept_<mode>/; root and <model> as artist_erasure.py forms them.
* Deviations from the reference: --batch_size is the classifier's batch (the reference samples `batch_size` images of the
  first prompt of a batch); with --dbg the accuracy is over the rows evaluated (the reference divides by all rows); labels
  are compared by ImageNet index (the ten class names are the torchvision category names, so the outcome is the same).
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from pdm.utils import erasure_utils as E
from pdm.utils import object_erasure as O
from pdm.utils.load_models import cuda_device, golden_path, inference_config
from pdm.utils.sld import sampling_kwargs


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--gpu', type=int, default=0)
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--dbg', action='store_true')
    parser.add_argument('--target', type=str, default=None)
    parser.add_argument('--baseline', type=str, default=None)
    parser.add_argument('--res_path', type=str, default='results/results_seed_0/stable-diffusion')
    parser.add_argument('--removal_mode', type=str, default=None, choices=['erase', 'keep'])
    parser.add_argument('--hook_module', type=str, default='unet')
    parser.add_argument('--model_id', type=str, default='stabilityai/stable-diffusion-2-1')
    parser.add_argument('--batch_size', type=int, default=64, help="classifier batch")
    parser.add_argument('--ckpt_name', type=str, default=None)
    # --- additions of this build (the loading / sampling flags of artist_erasure.py)
    parser.add_argument('--base_config_path', type=str)
    parser.add_argument('--original_ckpt', type=str, default=None)
    parser.add_argument('--result_dir', type=str, default=None, help="replaces results/results_seed_<seed>/<res_path part>")
    parser.add_argument('--image_resolution', type=int, default=768, help="when <model_id>/unet/config.json is absent")
    parser.add_argument('--num_inference_steps', type=int, default=50)
    parser.add_argument('--mixed_precision', type=str, default=None, choices=["no", "bf16"])
    parser.add_argument('--tiny', action="store_true", help="tiny U-Net topology (tests)")
    parser.add_argument('--sld_type', type=str, default=None, help="sample with this SLD preset")
    parser.add_argument('--sld_concept', type=str, default=None, help="SLD's safety concept (default: --target)")
    parser.add_argument('--prompts_csv', type=str, default=None, help="default: tests/golden/object_erasure/imagenette.csv")
    parser.add_argument('--resnet_weights', type=str, default=None, help="torchvision's resnet50-11ad3fa6.pth")
    parser.add_argument('--categories_file', type=str, default=None, help="1000 ImageNet category names (printed labels)")
    parser.add_argument('--resize_size', type=int, default=232)
    parser.add_argument('--crop_size', type=int, default=224)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    print("Arguments: ", args.__dict__)
    if args.target is None or args.baseline is None or args.removal_mode is None:
        raise ValueError("--target, --baseline and --removal_mode are required")
    E.check_baseline(args.baseline, args.ckpt_name)
    sld = None
    if args.sld_type is not None:
        sld = sampling_kwargs(args.sld_type, args.sld_concept if args.sld_concept is not None else args.target)
    if args.hook_module != "unet":
        raise NotImplementedError(f"--hook_module {args.hook_module}: only `unet` is built")
    categories = O.load_categories(args.categories_file) if args.categories_file else None
    O.label_index(args.target)                                     # an unknown class fails before anything is loaded
    directory = O.result_dir(args)
    print("Benchmarking result path: ", directory)
    os.makedirs(directory, exist_ok=True)
    rows = O.read_prompt_rows(args.prompts_csv or golden_path("object_erasure", "imagenette.csv"))
    selected = O.select_rows(rows, args.target, args.removal_mode, dbg=args.dbg)
    if not selected:
        raise ValueError(f"no rows to {args.removal_mode} for --target {args.target!r}")
    print("Number of prompts: ", len(selected))
    device = cuda_device(args.gpu)

    # Run the model if the folder is empty
    if len(os.listdir(directory)) == 0:
        if args.original_ckpt is None:
            raise ValueError("generation needs --original_ckpt")
        config = inference_config(args.base_config_path, args.model_id, args.tiny, args.mixed_precision)
        original, erased = E.load_pipelines(config, args, device)
        del original
        O.generate(selected, directory, erased, E.image_resolution(args.model_id, args.image_resolution),
                   args.num_inference_steps, sld=sld)
        del erased

    from pdm.models.resnet import ResNet50Classifier
    classifier = ResNet50Classifier.from_pretrained(args.resnet_weights, device=device)
    hits, n, predicted = O.score_folder(selected, directory, classifier, batch_size=args.batch_size, resize_size=args.resize_size,
                                        crop_size=args.crop_size, with_predictions=True)
    for (prompt, seed, label), j in zip(selected, predicted):
        print(f"Predicted labels: {[O.category_name(j, categories)]}", "True label: ", label)
    print("Object predicted in: %d/%d images" % (hits, n))
    print(f"Average accuracy: {hits / n}")
    results, _ = O.write_result(directory, args.removal_mode, args.ckpt_name, hits, n)
    return results


if __name__ == '__main__':
    main()
