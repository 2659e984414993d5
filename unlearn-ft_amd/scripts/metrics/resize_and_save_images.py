"""Resize every image of a directory to --size W H and save it as <stem>.npy (uint8 [H, W, 3]) - the reference's
scripts/metrics/resize_and_save_images.py, with Pillow's default 8-bpc bicubic `Image.resize` computed on the GPU
(pdmk_image_resize_u8, bit-exact with Pillow).  Deviation: the output stem is os.path.splitext(name)[0], where the reference
cuts the last four characters (`img_name[:-4]`, which mangles `.jpeg` / `.webp` names)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Resize images in a directory")
    parser.add_argument("--data_dir", type=str, required=True, help="Directory containing images")
    parser.add_argument("--output_dir", type=str, required=True, help="Directory to save resized images")
    parser.add_argument("--size", type=int, nargs=2, default=[512, 512], help="Size of the resized images (W H)")
    parser.add_argument("--batch_size", type=int, default=16)
    parser.add_argument("--num_workers", type=int, default=None)
    return parser.parse_args(argv)


def output_name(img_name):
    return os.path.splitext(img_name)[0] + ".npy"


class _Batches(torch.utils.data.Dataset):
    def __init__(self, data_dir, names, batch_size):
        self.dir, self.names, self.bs = data_dir, names, int(batch_size)

    def __len__(self):
        return -(-len(self.names) // self.bs)

    def __getitem__(self, b):
        from pdm.utils.clip_utils import load_image
        from pdm.utils.fid_utils import pack_images
        names = self.names[b * self.bs:(b + 1) * self.bs]
        packed, desc = pack_images([load_image(os.path.join(self.dir, n)) for n in names])
        return {"packed": packed, "image_desc": desc, "names": names}


def resize_batch(packed, desc, size, device):
    """Packed host batch -> uint8 [B, H, W, 3] on the device, each image resized to size = (W, H)."""
    from pdm import _pdmk
    from pdm.utils.data import upload
    B = desc.shape[0]
    desc = desc.clone()
    desc[:, 3], desc[:, 4] = size[1], size[0]
    src, _ = upload(packed, B, device)                  # the descriptors in the buffer carry no target size
    out = torch.empty(B, size[1], size[0], 3, device=device, dtype=torch.uint8)
    _pdmk.image_resize_u8(src, desc, desc.to(device), out)
    return out


def resize_images_in_dir(data_dir, output_dir, size, batch_size=16, num_workers=None, device="cuda:0"):
    from pdm.utils.clip_utils import default_workers
    names = sorted(n for n in os.listdir(data_dir) if not n.startswith("."))
    dl = torch.utils.data.DataLoader(_Batches(data_dir, names, batch_size), batch_size=None, shuffle=False,
                                     num_workers=default_workers(num_workers))
    for batch in dl:
        out = resize_batch(batch["packed"], batch["image_desc"], size, device).cpu().numpy()
        for img, name in zip(out, batch["names"]):
            np.save(os.path.join(output_dir, output_name(name)), img)


def main(argv=None):
    args = parse_args(argv)
    if not os.path.exists(args.output_dir):
        os.makedirs(args.output_dir)
    resize_images_in_dir(args.data_dir, args.output_dir, size=tuple(args.size), batch_size=args.batch_size,
                         num_workers=args.num_workers)


if __name__ == "__main__":
    main()
