"""Caption files of the CLIP score (the reference's scripts/metrics/save_captions.py, COCO writer): one
<annotations dir>/clip-captions/<image id>.txt per caption of --annotations_file, named COCO_<split>_%012d for 2014 files
and %012d otherwise.  An image with several captions keeps the last one, as in the reference."""
import argparse
import json
import os


def caption_name(annotations_file, image_id):
    split_name = os.path.basename(annotations_file)[len('captions_'):-len('.json')]
    if '2014' in annotations_file:
        return f"COCO_{split_name}_%012d" % image_id
    return "%012d" % image_id


def save_coco_captions(annotations_file):
    with open(annotations_file) as f:
        captions_file = json.load(f)
    save_dir = os.path.join(os.path.dirname(annotations_file), 'clip-captions')
    os.makedirs(save_dir, exist_ok=True)
    for capt in captions_file['annotations']:
        with open(os.path.join(save_dir, caption_name(annotations_file, capt['image_id']) + '.txt'), 'w') as f:
            f.write(capt['caption'])
    return save_dir


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--annotations_file', type=str, required=True,
                        help="COCO captions json, e.g. annotations/captions_val2014_30k.json")
    return save_coco_captions(parser.parse_args(argv).annotations_file)


if __name__ == '__main__':
    main()
