#!/usr/bin/env python3
"""LPIPS (AlexNet, lpips v0.1) between the images of the original and of the edited model, with the reference's name and flags
(baselines/unified-concept-editing/eval-scripts/lpips_eval.py, the same file under baselines/erasing/oldcode_erasing_compvis):
    python scripts/baselines/unified_concept_editing/lpips_eval.py --original_path OUT/original --edited_path OUT/<edit> \\
        --csv_path tests/golden/artist_prompts/test_Van\\ Gogh.csv --save_path OUT \\
        [--alexnet_weights alexnet-owt-7be5be79.pth --lpips_weights alex.pth]

* Per row of --csv_path: the files `<case_number>_<n>.png` of --original_path, each against the file of the same name in
  --edited_path (a missing one is printed and skipped), Resize(--imsize) + ToTensor, scaled to [-1, 1]; `lpips_loss` is the mean
  over the case's files, NaN for a case without files.  Output: <save_path>/<basename(edited_path)>_lpipsloss.csv (the last
  component before a trailing slash), the prompts frame plus `lpips_loss`.
* Weights: torchvision's AlexNet and lpips' weights/v0.1/alex.pth from the flags or torch hub's checkpoint cache; nothing is
  downloaded.  The trunk and the metric head run on the GPU (pdm/models/perceptual), all pairs of the folder in batches.
* Deviations from the reference: its --image branch calls a function the file never defines; here --image takes the two paths
  as single files and writes `filename, lpips_loss` to --save_path.  Images are read as RGB.  Only square images.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from pdm.utils import perceptual as P


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='LPIPS', description='Takes the path to two images and gives LPIPS')
    parser.add_argument('--original_path', help='path to original image', type=str, required=True)
    parser.add_argument('--edited_path', help='path to edited image', type=str, required=True)
    parser.add_argument('--csv_path', help='path to csv prompts', type=str, required=False, default=None)
    parser.add_argument('--save_path', help='path to save results', type=str, required=False, default=None)
    parser.add_argument("--image", action="store_true", help="Whether it is a single image path")
    parser.add_argument('--imsize', type=int, default=64, help="Resize(imsize) of both images (the reference's value)")
    parser.add_argument('--alexnet_weights', type=str, default=None, help="torchvision's alexnet-owt-7be5be79.pth")
    parser.add_argument('--lpips_weights', type=str, default=None, help="lpips' weights/v0.1/alex.pth")
    parser.add_argument('--batch_size', type=int, default=64, help="pairs per launch")
    parser.add_argument('--device', type=str, default='cuda:0')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if not args.image and args.csv_path is None:
        raise ValueError("--csv_path is required unless --image is given")
    from pdm.models.perceptual import AlexNetLPIPS
    model = AlexNetLPIPS.from_pretrained(args.alexnet_weights, args.lpips_weights, device=args.device)

    def metric(a, b):
        return P.lpips_distance(a, b, model, imsize=args.imsize, batch_size=args.batch_size)

    if args.image:
        value = float(metric([args.original_path], [args.edited_path])[0])
        print(f'LPIPS score: {value}')
        if args.save_path is not None:
            P.write_frame(args.save_path, ["filename", "lpips_loss"], [[args.edited_path.split('/')[-1], value]])
        return value
    header, rows = P.evaluate_folders(args.original_path, args.edited_path, args.csv_path, ["lpips_loss"], metric)
    if args.save_path is not None:
        return P.write_frame(P.result_csv(args.save_path, args.edited_path, "lpipsloss"), header, rows)
    return header, rows


if __name__ == '__main__':
    main()
