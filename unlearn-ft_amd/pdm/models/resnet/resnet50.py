"""`ResNet50Classifier`: torchvision's `resnet50` (v1.5) on libpdmk - the classifier of the object-erasure evaluation
(pdm/utils/object_erasure.py).  fp32, inference only, NHWC; a `ConvTrunk` (pdm/models/convnet.py): one fp32 weight arena,
BatchNorm folded into weight and bias in float64 on the host, every conv one launch, eager on the current stream.

conv1 (7 x 7 / 2, ReLU fused) -> pdmk_pool2d (max, 3 x 3 / 2 / pad 1) -> the bottlenecks -> pdmk_global_avgpool -> fc as a
1 x 1 pdmk_conv2d_fwd on the [B, 2048] map -> pdmk_softmax_topk.  A bottleneck is conv1 (1 x 1, ReLU), conv2 (3 x 3 / s,
ReLU), the downsample conv where the block has one (1 x 1 / s, no ReLU, its own buffer), and conv3 through
pdmk_conv2d_fwd_res: the residual - the downsample output or the block's input - is added in conv3's epilogue before the
ReLU.  An identity block writes conv3 over its input buffer (res == y): the trunk holds one block-output buffer per stage.

`classify` prepares images as torchvision's ImageClassification preset does on a PIL image: Pillow's bilinear resize of the
short side to resize_size, centre crop, / 255, ImageNet normalisation (pdmk_image_prep_ex, filter 0, bit for bit), then
pdmk_nchw_to_nhwc.  That reading of the preset and the real IMAGENET1K_V2 weights are unchecked: torchvision is not on the
build machine.
"""
import os

import numpy as np
import torch

from ... import _pdmk as k
from ..convnet import ConvTrunk, Map, checked, fold_unit, hub_checkpoint, load_weights_file
from . import spec as S

WEIGHTS_NAME = "resnet50-11ad3fa6.pth"          # IMAGENET1K_V2: what ResNet50_Weights.DEFAULT names
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MIN_SIZE = 32


def default_weights_path():
    """Where torch hub keeps torchvision's ResNet-50 weights."""
    return hub_checkpoint(WEIGHTS_NAME)


def _load_image(image):
    """(name, uint8 [H, W, 3]) of an array or a file read as Image.open(...).convert("RGB")."""
    if isinstance(image, (str, os.PathLike)):
        from PIL import Image
        with Image.open(image) as im:
            return str(image), np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8))
    a = np.ascontiguousarray(torch.as_tensor(image).cpu().numpy() if torch.is_tensor(image) else np.asarray(image))
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"expected a uint8 [H, W, 3] image, got {a.dtype} {a.shape}")
    return "array", a


class ResNet50Classifier(ConvTrunk):
    def __init__(self, device=None, seed=0, init=True, layers=(3, 4, 6, 3)):
        self.layers = tuple(layers)
        self.convs = S.build_units(self.layers)             # the conv + BatchNorm units; `units` has fc behind them
        super().__init__(device, self.convs + [S.FC])
        if init:
            self.load_state_dict(S.init_state_dict(seed, self.convs))

    @classmethod
    def from_pretrained(cls, path=None, device=None):
        """The weights file given, else torch hub's cache; never fetched."""
        sd = load_weights_file(path, WEIGHTS_NAME, "--resnet_weights", "torchvision ResNet-50")
        model = cls(device=device, init=False)
        model.load_state_dict(sd)
        return model

    def load_state_dict(self, sd):
        """torchvision's keys; num_batches_tracked is ignored, a missing / mis-shaped key raises."""
        sd = checked(sd, S.state_dict_shapes(self.convs, num_batches_tracked=False), "ResNet", S.ignored)
        host = torch.zeros(self.arena.numel(), dtype=torch.float32)
        for u in self.convs:
            self.fill_conv(host, u, *fold_unit(sd, *S.keys(u), S.BN_EPS))
        self.fill_conv(host, S.FC, sd["fc.weight"], sd["fc.bias"])
        self.arena.copy_(host)

    def bottleneck(self, x, p):
        """relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + shortcut(x)).  Without a downsample conv the result
        overwrites x's buffer."""
        t = self.conv(self.conv(x, f"{p}.conv1", True), f"{p}.conv2", True)
        if f"{p}.downsample.0" in self.units:
            short = self.conv(x, f"{p}.downsample.0", False)
            return self.conv(t, f"{p}.conv3", True, res=short)
        return self.conv(t, f"{p}.conv3", True, res=x, out=x)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward_nhwc(self, x):
        """x fp32 [B, H, W, 3], ImageNet-normalised, on the device, H, W >= 32 -> logits [B, 1000] fp32."""
        B, H, W, C = x.shape
        assert C == 3 and x.dtype == torch.float32 and x.is_contiguous() and min(H, W) >= MIN_SIZE, tuple(x.shape)
        m = self.pool(self.conv(Map(x.reshape(B * H * W, 3), B, H, W), "conv1", True), "max", 2, 1)
        for l, n in enumerate(self.layers, start=1):
            for i in range(n):
                m = self.bottleneck(m, f"layer{l}.{i}")
        feat = torch.empty((B, m.C), device=self.device, dtype=torch.float32)
        k.global_avgpool(m.t, m.ld, feat, B, m.H * m.W, m.C)
        return self.conv(Map(feat, B, 1, 1), S.FC, False).t

    @torch.no_grad()
    def prep(self, images, resize_size=232, crop_size=224):
        """uint8 [H, W, 3] arrays or paths -> the normalised fp32 NHWC batch [B, crop, crop, 3]: Pillow's bilinear resize of
        the short side to resize_size (the long side int(resize_size * long / short)), centre crop at
        int(round((side - crop) / 2.0)), / 255, ImageNet Normalize."""
        from ...utils.data import center_crop_origin, pack_images, prep_nhwc, resized_size
        R = int(crop_size)
        rows, arrays = [], []
        for image in images:
            name, a = _load_image(image)
            h, w = a.shape[:2]
            rh, rw = resized_size(h, w, int(resize_size))
            if min(rh, rw) < R:
                raise ValueError(f"{name}: {w} x {h} resizes to {rw} x {rh}, smaller than the {R} x {R} crop")
            rows.append([h, w, rh, rw, *center_crop_origin(rh, rw, R), 0])
            arrays.append(a)
        assert arrays, "no images"
        packed, desc = pack_images(arrays, rows)
        return prep_nhwc(packed, desc, R, self.device, 0, IMAGENET_MEAN, IMAGENET_STD)

    @torch.no_grad()
    def classify(self, images, topk=5, resize_size=232, crop_size=224, batch_size=250):
        """Top-k classes of every image: (probs fp32 [N, k], idx int64 [N, k]) on the host, most probable first, equal
        probabilities lower index first.  images: uint8 [H, W, 3] arrays or paths (any sizes), run in batches."""
        images = list(images)
        if int(crop_size) < MIN_SIZE:
            raise ValueError(f"crop_size {crop_size} is below the network's minimum of {MIN_SIZE}")
        probs, idx = [], []
        for i in range(0, len(images), int(batch_size)):
            logits = self.forward_nhwc(self.prep(images[i:i + int(batch_size)], resize_size, crop_size))
            p, j = k.softmax_topk(logits, int(topk))
            probs.append(p.cpu())
            idx.append(j.cpu().to(torch.int64))
        if not probs:
            return torch.zeros(0, int(topk)), torch.zeros(0, int(topk), dtype=torch.int64)
        return torch.cat(probs), torch.cat(idx)
