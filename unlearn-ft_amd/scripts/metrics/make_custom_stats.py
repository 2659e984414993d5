"""Real-image statistics for fid.py: the reference README's `fid.make_custom_stats(dataset, dataset_path,
mode="legacy_pytorch")` as a script.  Writes {stats_dir}/{name}_{mode}_custom_na.npz (mu [2048], sigma [2048, 2048])."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from pdm.utils.fid_utils import make_custom_stats

logging.basicConfig(level=logging.INFO)


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--name', type=str, required=True, help="dataset name, e.g. coco-30k")
    parser.add_argument('--data_dir', type=str, required=True, help="the real images (.npy uint8 [H, W, 3] or image files)")
    parser.add_argument('--mode', type=str, default="legacy_pytorch")
    parser.add_argument('--stats_dir', type=str, default=None, help="default: $PDM_FID_STATS or ~/.cache/pdm/fid_stats")
    parser.add_argument('--inception_weights', type=str, default=None,
                        help="pt_inception-2015-12-05-6726825d.pth (default: torch hub's checkpoint cache)")
    parser.add_argument('--batch_size', type=int, default=64)
    parser.add_argument('--num_workers', type=int, default=None)
    return parser.parse_args(argv)


def main(argv=None, model=None):
    args = parse_args(argv)
    return make_custom_stats(args.name, args.data_dir, mode=args.mode, stats_dir=args.stats_dir, model=model,
                             inception_weights=args.inception_weights, batch_size=args.batch_size,
                             num_workers=args.num_workers)


if __name__ == '__main__':
    main()
