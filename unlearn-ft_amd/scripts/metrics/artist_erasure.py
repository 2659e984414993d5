#!/usr/bin/env python3
"""Artist-erasure score with the reference's name and flags (baselines/concept_prune/artist_erasure.py:20-34, run by
eval_artish.sh with `--baseline pdm`): did the bilevel fine-tuning erase the artist?
    python scripts/metrics/artist_erasure.py --target "Van Gogh" --baseline pdm --base_config_path CFG \\
        --model_id <SD-2.1 snapshot> --original_ckpt <pruned>/checkpoint-N/ --ckpt_name <erased>/checkpoint-M/ \\
        --clip_model <clip-vit-base-patch32 directory or ViT-B-32.pt> [--mixed_precision bf16]

* Prompts: the `prompt` column of --prompts_csv (default tests/golden/artist_prompts/test_<target>.csv, the reference's
  datasets/test_<target>.csv); `evaluation_seed` is read and ignored, the reference overwrites it with 0.
* Generation, only when the image directory is empty (as the reference): per prompt the initial latents are drawn once from
  `torch.Generator(device).manual_seed(seed)` and the text encoder runs once; the original pipeline (--original_ckpt) and the
  erased one get the same latents and embeddings.  50 steps, guidance 7.5, PNDM from the snapshot, at sample_size x 8 of
  <model_id>/unet/config.json (768 for SD-2.1; without that file --image_resolution).  uint8 as diffusers' numpy_to_pil
  (rounded: pdmk_image_to_u8_ex), `original_{i}.jpg` / `removal_{i}.jpg` by Pillow's default save.  The two loops run one
  after the other.
* --baseline: `pdm` = <ckpt_name>/arch_vector.pt + unet/diffusion_pytorch_model.safetensors; `pruned_baseline` = the
  original checkpoint itself; `esd` / `uce` = the original checkpoint with the erasure checkpoint --ckpt_name laid over it
  (ESD: nested {module: {weight, bias}}, non-strict; UCE: a full state dict, strict); `concept-prune` = the same with the
  checkpoint scripts/baselines/concept_prune/save_union_over_time.py writes (a full state dict, strict; its masked layers are
  fp16; without --ckpt_name it raises NotImplementedError: the reference's table of checkpoint paths is not built).
  `concept-ablation` and `baseline` raise NotImplementedError.
* Scoring, always, from the files: CLIP ViT-B/32 (--clip_model, resolved like clip_score.py's: a local transformers
  directory or an OpenAI .pt; a hub id raises FileNotFoundError) in fp32 (--mixed_precision is the samplers' dtype) of
  prompt and images, pdmk_cosine_pairs per batch of --batch_size pairs, then
  numpy as the reference: avg / std of cos(prompt, erased image), avg / std of the 0/1 flags "erased image less similar
  than the original".  Written as JSON to <images>/clip_scores_<p>_VG.json and returned from main(argv).
* Result path: <--result_dir or results/results_seed_<seed>/<res_path.split('/')[2]>>/<model>/<target>/<baseline>/
  benchmarking/concept_erase/<run_ckpt>/concept_erase/.  Deviations from the reference: <model> is model_id, or its
  basename when it is an existing local path; <run_ckpt> is the last two components of the normalised
  `ckpt_name or original_ckpt` (the reference indexes split('/') and so needs the trailing slash); <p> is the basename of
  the normalised ckpt_name without `.pt`; the reference's own root is the placeholder `path/to/concept_prune/results`.
  --model_id defaults to SD-2.1 (what eval_artish.sh passes), not the reference's SD-1.4.
* --sld_type Weak|Medium|Strong|Max [--sld_concept TEXT, default --target]: the removal images are sampled with Safe Latent
  Diffusion (configs/baselines/sld.yaml, pdm/utils/sld.py) on whatever model --baseline selects; the original images are not.
  The <baseline> component of the result path becomes <baseline>_SLD_<type>.
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from pdm.utils import erasure_utils as E
from pdm.utils.load_models import cuda_device, inference_config
from pdm.utils.sld import sampling_kwargs


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--gpu', type=int, default=0)
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--dbg', type=bool, default=None)
    parser.add_argument('--target', type=str, default=None)
    parser.add_argument('--baseline', type=str, default=None)
    parser.add_argument('--hook_module', type=str, default='unet')
    parser.add_argument('--ckpt_name', type=str, default=None)
    parser.add_argument('--model_id', type=str, default='stabilityai/stable-diffusion-2-1')
    parser.add_argument('--res_path', type=str, default='results/results_seed_0/stable-diffusion/')
    parser.add_argument('--base_config_path', type=str)
    parser.add_argument('--original_ckpt', type=str, default=None)
    # --- additions of this build
    parser.add_argument('--prompts_csv', type=str, default=None, help="default: tests/golden/artist_prompts/test_<target>.csv")
    parser.add_argument('--result_dir', type=str, default=None, help="replaces results/results_seed_<seed>/<res_path part>")
    parser.add_argument('--clip_model', type=str, default="openai/clip-vit-base-patch32")
    parser.add_argument('--tokenizer', type=str, default=None, help="CLIP tokenizer directory (default: --clip_model's)")
    parser.add_argument('--image_resolution', type=int, default=768, help="when <model_id>/unet/config.json is absent")
    parser.add_argument('--num_inference_steps', type=int, default=50)
    parser.add_argument('--mixed_precision', type=str, default=None, choices=["no", "bf16"])
    parser.add_argument('--tiny', action="store_true", help="tiny U-Net topology (tests)")
    parser.add_argument('--batch_size', type=int, default=64, help="scoring batch")
    parser.add_argument('--sld_type', type=str, default=None, help="sample the removal images with this SLD preset")
    parser.add_argument('--sld_concept', type=str, default=None, help="SLD's safety concept (default: --target)")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    print("Arguments: ", args.__dict__)
    if args.target is None or args.baseline is None:
        raise ValueError("--target and --baseline are required")
    E.check_baseline(args.baseline, args.ckpt_name)
    sld = None
    if args.sld_type is not None:
        sld = sampling_kwargs(args.sld_type, args.sld_concept if args.sld_concept is not None else args.target)
    if args.hook_module != "unet":
        raise NotImplementedError(f"--hook_module {args.hook_module}: only `unet` is built")
    if args.ckpt_name is None and args.original_ckpt is None:
        raise ValueError("pass --original_ckpt (and --ckpt_name for pdm / esd / uce)")
    directory = E.images_dir(args)
    print("Benchmarking result path: ", os.path.dirname(directory))
    os.makedirs(directory, exist_ok=True)
    prompts = E.read_prompts(args.prompts_csv or E.default_prompts_csv(args.target))
    device = cuda_device(args.gpu)

    # Run the models if the folder is empty
    if len(os.listdir(directory)) == 0:
        print("Saving images after removal of concept")
        if args.original_ckpt is None:
            raise ValueError("generation needs --original_ckpt")
        config = inference_config(args.base_config_path, args.model_id, args.tiny, args.mixed_precision)
        original, erased = E.load_pipelines(config, args, device)
        E.generate(prompts, directory, original, erased, args.seed, E.image_resolution(args.model_id, args.image_resolution),
                   args.num_inference_steps, sld=sld)
        del original, erased

    print("Calculating CLIP scores for the images")
    results = E.score(prompts, directory, args.clip_model, tokenizer=args.tokenizer, batch_size=args.batch_size, device=device)
    print(f"Average similarity between prompt and generated image after removal: {results['avg_similarity']}")
    print(f"Average score between prompt and generated image after removal: {results['avg_score']}")
    E.write_result(directory, args.ckpt_name, results)
    return results


if __name__ == '__main__':
    main()
