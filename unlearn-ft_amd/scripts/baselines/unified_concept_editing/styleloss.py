#!/usr/bin/env python3
"""VGG-19 Gram-matrix style loss and content loss between the images of the original and of the edited model, with the
reference's name and flags (baselines/unified-concept-editing/eval-scripts/styleloss.py, the same file under
baselines/erasing/oldcode_erasing_compvis):
    python scripts/baselines/unified_concept_editing/styleloss.py --original_path OUT/original --edited_path OUT/<edit> \\
        --csv_path tests/golden/artist_prompts/test_Van\\ Gogh.csv --save_path OUT [--vgg_weights vgg19-dcbb9e9d.pth]

* The original is the style and the content image, the edited one the input: style = sum over conv_1 .. conv_5 (pre-ReLU) of
  mse(Gram(edited), Gram(original)), content = mse at conv_4, total = 1e6 style + content.
* Per row of --csv_path: the files `<case_number>_<n>.png` of --original_path against the same names in --edited_path (a missing
  one is printed and skipped), Resize(--imsize) + ToTensor; `style_loss, content_loss, total_loss` are the means over the case's
  files, NaN for a case without files.  Output: <save_path>/<basename(edited_path)>_styleloss.csv.
* Weights: torchvision's VGG-19 from --vgg_weights or torch hub's checkpoint cache; nothing is downloaded.
* Deviations from the reference: images are read as RGB (it feeds whatever mode the file has); a missing edited file is
  skipped as lpips_eval.py does (here the reference stops); a trailing slash of --edited_path is handled as lpips_eval.py does;
  --image writes `filename, Style_Loss, Content_Loss, Total_Loss` to --save_path; only square images.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from pdm.utils import perceptual as P


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog='StyleLoss',
                                     description='Takes the path to two images and gives Style and Content Loss. 0 means identical')
    parser.add_argument('--original_path', help='path to original image', type=str, required=True)
    parser.add_argument('--edited_path', help='path to edited image', type=str, required=True)
    parser.add_argument('--csv_path', help='path to csv prompts', type=str, required=False, default=None)
    parser.add_argument('--save_path', help='path to save results', type=str, required=False, default=None)
    parser.add_argument("--image", action="store_true", help="Whether it is a single image path")
    parser.add_argument('--imsize', type=int, default=512, help="Resize(imsize) of both images (the reference's GPU value)")
    parser.add_argument('--vgg_weights', type=str, default=None, help="torchvision's vgg19-dcbb9e9d.pth")
    parser.add_argument('--batch_size', type=int, default=8, help="pairs per launch")
    parser.add_argument('--device', type=str, default='cuda:0')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if not args.image and args.csv_path is None:
        raise ValueError("--csv_path is required unless --image is given")
    from pdm.models.perceptual import VGG19Style
    model = VGG19Style.from_pretrained(args.vgg_weights, device=args.device)

    def metric(a, b):
        return P.style_content_loss(a, b, model, imsize=args.imsize, batch_size=args.batch_size)

    if args.image:
        style, content, total = (float(v[0]) for v in metric([args.original_path], [args.edited_path]))
        print(f'Style Loss: {style} \t Content Loss: {content} \t Total Loss: {total}')
        if args.save_path is not None:
            P.write_frame(args.save_path, ["filename", "Style_Loss", "Content_Loss", "Total_Loss"],
                          [[args.edited_path.split('/')[-1], style, content, total]])
        return style, content, total
    header, rows = P.evaluate_folders(args.original_path, args.edited_path, args.csv_path,
                                      ["style_loss", "content_loss", "total_loss"], metric)
    if args.save_path is not None:
        return P.write_frame(P.result_csv(args.save_path, args.edited_path, "styleloss"), header, rows)
    return header, rows


if __name__ == '__main__':
    main()
