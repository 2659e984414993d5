"""FID of generated images (the reference's scripts/metrics/fid.py, same flags): appends "{gen_dir} {fid}" to
{result_dir}/fid.txt.  The real-image statistics come from make_custom_stats.py ({stats_dir}/{dataset}_{mode}_custom_na.npz);
--stats_dir, --inception_weights, --batch_size, --num_workers are local additions.  Nothing is downloaded."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from pdm.utils.fid_utils import compute_fid

logging.basicConfig(level=logging.INFO)


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--gen_dir', type=str, required=True)
    parser.add_argument('--dataset', type=str, default="coco-30k")
    parser.add_argument('--mode', type=str, default="legacy_pytorch")
    parser.add_argument('--result_dir', type=str, required=True, help="Directory to save the results")
    parser.add_argument('--stats_dir', type=str, default=None, help="default: $PDM_FID_STATS or ~/.cache/pdm/fid_stats")
    parser.add_argument('--inception_weights', type=str, default=None,
                        help="pt_inception-2015-12-05-6726825d.pth (default: torch hub's checkpoint cache)")
    parser.add_argument('--batch_size', type=int, default=64)
    parser.add_argument('--num_workers', type=int, default=None)
    return parser.parse_args(argv)


def result_file(result_dir):
    return f"{result_dir}/fid.txt"


def write_result(result_dir, gen_dir, fid_value):
    os.makedirs(result_dir, exist_ok=True)
    with open(result_file(result_dir), "a") as f:
        f.write(f"{gen_dir} {fid_value}\n")


def main(argv=None, model=None):
    args = parse_args(argv)
    fid_value = compute_fid(args.gen_dir, dataset_name=args.dataset, mode=args.mode, dataset_split="custom",
                            stats_dir=args.stats_dir, model=model, inception_weights=args.inception_weights,
                            batch_size=args.batch_size, num_workers=args.num_workers)
    logging.info(f"FID: {fid_value}")
    write_result(args.result_dir, args.gen_dir, fid_value)
    return fid_value


if __name__ == '__main__':
    main()
