"""`ResNet50Classifier`: torchvision's `resnet50` (v1.5) on libpdmk - the classifier of the object-erasure evaluation
(pdm/utils/object_erasure.py).  fp32, inference only, NHWC; the pattern of pdm/models/inception: one fp32 weight arena,
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
from ..inception.inception_v3 import _Map
from .spec import NUM_CLASSES, build_units, checked_trunk, fold_batchnorm, init_state_dict

WEIGHTS_NAME = "resnet50-11ad3fa6.pth"          # IMAGENET1K_V2: what ResNet50_Weights.DEFAULT names
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MIN_SIZE = 32


def default_weights_path():
    """Where torch hub keeps torchvision's ResNet-50 weights."""
    return os.path.join(os.path.expanduser("~"), ".cache", "torch", "hub", "checkpoints", WEIGHTS_NAME)


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


class ResNet50Classifier:
    def __init__(self, device=None, seed=0, init=True, layers=(3, 4, 6, 3)):
        if not torch.cuda.is_available():
            raise RuntimeError("ResNet50Classifier (MI355X engine) needs a GPU; there is no CPU fallback")
        self.device = torch.device(device or "cuda:0")
        self.layers = tuple(layers)
        self.units = {u.name: u for u in build_units(self.layers)}
        self.fc_in = self.units[f"layer4.{self.layers[3] - 1}.conv3"].co
        off, self.offsets = 0, {}
        sizes = [(u.name, u.co, u.k) for u in self.units.values()] + [("fc", NUM_CLASSES, self.fc_in)]
        for name, co, kk in sizes:                          # weight [Co, kh * kw * Ci] then bias [Co], each on a 512-byte line
            self.offsets[name] = (off, off + (co * kk + 127) // 128 * 128)
            off = self.offsets[name][1] + (co + 127) // 128 * 128
        self.arena = torch.zeros(off, device=self.device, dtype=torch.float32)
        if init:
            self.load_state_dict(init_state_dict(seed, list(self.units.values())))

    @classmethod
    def from_pretrained(cls, path=None, device=None):
        """The weights file given, else torch hub's cache; never fetched."""
        path = path or default_weights_path()
        if not os.path.isfile(path):
            raise FileNotFoundError(f"ResNet-50 weights not found at {path}: place torchvision's {WEIGHTS_NAME} there or pass "
                                    f"--resnet_weights FILE (nothing is downloaded)")
        sd = torch.load(path, map_location="cpu", weights_only=True)
        model = cls(device=device, init=False)
        model.load_state_dict(sd)
        return model

    def load_state_dict(self, sd):
        """torchvision's keys; num_batches_tracked is ignored, a missing / mis-shaped key raises."""
        sd = checked_trunk(sd, list(self.units.values()))
        host = torch.zeros(self.arena.numel(), dtype=torch.float32)
        for u in self.units.values():
            w, b = fold_batchnorm(sd[f"{u.conv}.weight"], sd[f"{u.bn}.weight"], sd[f"{u.bn}.bias"],
                                  sd[f"{u.bn}.running_mean"], sd[f"{u.bn}.running_var"])
            wo, bo = self.offsets[u.name]
            host[wo:wo + u.co * u.k] = w.permute(0, 2, 3, 1).reshape(-1).to(torch.float32)       # k = (ky, kx, ci)
            host[bo:bo + u.co] = b.to(torch.float32)
        wo, bo = self.offsets["fc"]
        host[wo:wo + NUM_CLASSES * self.fc_in] = sd["fc.weight"].detach().reshape(-1).to(torch.float32)
        host[bo:bo + NUM_CLASSES] = sd["fc.bias"].detach().to(torch.float32)
        self.arena.copy_(host)

    # ------------------------------------------------------------------ ops
    def _new(self, B, H, W, C):
        return _Map(torch.empty((B * H * W, C), device=self.device, dtype=torch.float32), B, H, W)

    def conv(self, x, name, relu, res=None, out=None):
        """One launch: the unit's conv + folded BatchNorm (+ res) (+ ReLU).  out: the map to write (it may be res)."""
        u = self.units[name]
        assert x.C == u.ci, (name, x.C, u.ci)
        Ho, Wo = (x.H + 2 * u.ph - u.kh) // u.stride + 1, (x.W + 2 * u.pw - u.kw) // u.stride + 1
        y = out if out is not None else self._new(x.B, Ho, Wo, u.co)
        assert (y.B, y.H, y.W, y.C) == (x.B, Ho, Wo, u.co), (name, y.H, y.W, y.C)
        wo, bo = self.offsets[name]
        w, b = self.arena[wo:wo + u.co * u.k], self.arena[bo:bo + u.co]
        if res is None:
            k.conv2d_fwd(x.t, x.ld, w, b, y.t, y.ld, x.B, x.H, x.W, u.ci, u.co, u.kh, u.kw, u.stride, u.ph, u.pw, relu=relu)
        else:
            assert (res.B, res.H, res.W, res.C) == (y.B, y.H, y.W, y.C), name
            k.conv2d_fwd_res(x.t, x.ld, w, b, res.t, res.ld, y.t, y.ld, x.B, x.H, x.W, u.ci, u.co, u.kh, u.kw, u.stride, u.ph,
                             u.pw, relu=relu)
        return y

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
        m = self.conv(_Map(x.reshape(B * H * W, 3), B, H, W), "conv1", True)
        pooled = self._new(B, (m.H - 1) // 2 + 1, (m.W - 1) // 2 + 1, m.C)
        k.pool2d(m.t, m.ld, pooled.t, pooled.ld, B, m.H, m.W, m.C, "max", 2, 1)
        m = pooled
        for l, n in enumerate(self.layers, start=1):
            for i in range(n):
                m = self.bottleneck(m, f"layer{l}.{i}")
        feat = torch.empty((B, m.C), device=self.device, dtype=torch.float32)
        k.global_avgpool(m.t, m.ld, feat, B, m.H * m.W, m.C)
        logits = torch.empty((B, NUM_CLASSES), device=self.device, dtype=torch.float32)
        wo, bo = self.offsets["fc"]
        k.conv2d_fwd(feat, m.C, self.arena[wo:wo + NUM_CLASSES * m.C], self.arena[bo:bo + NUM_CLASSES], logits, NUM_CLASSES,
                     B, 1, 1, m.C, NUM_CLASSES, 1, 1, 1, 0, 0, relu=False)
        return logits

    @torch.no_grad()
    def prep(self, images, resize_size=232, crop_size=224):
        """uint8 [H, W, 3] arrays or paths -> the normalised fp32 NHWC batch [B, crop, crop, 3]: Pillow's bilinear resize of
        the short side to resize_size (the long side int(resize_size * long / short)), centre crop at
        int(round((side - crop) / 2.0)), / 255, ImageNet Normalize."""
        from ...utils.clip_utils import DESC_BYTES
        from ...utils.data import center_crop_origin, resized_size
        R = int(crop_size)
        desc, arrays, off = [], [], 0
        for image in images:
            name, a = _load_image(image)
            h, w = a.shape[:2]
            rh, rw = resized_size(h, w, int(resize_size))
            if min(rh, rw) < R:
                raise ValueError(f"{name}: {w} x {h} resizes to {rw} x {rh}, smaller than the {R} x {R} crop")
            top, left = center_crop_origin(rh, rw, R)
            desc.append([off, h, w, rh, rw, top, left, 0])
            arrays.append(a)
            off += (a.size + 3) & ~3
        assert arrays, "no images"
        n, head = len(arrays), len(arrays) * DESC_BYTES
        packed = torch.zeros(head + off + 4, dtype=torch.uint8)
        buf = packed.numpy()
        d = np.asarray(desc, np.int64).reshape(n, 8)
        buf[:head] = d.reshape(-1).view(np.uint8)
        for (o, *_), a in zip(desc, arrays):
            buf[head + o:head + o + a.size] = a.reshape(-1)
        dev = packed.to(self.device, non_blocking=True)
        pix = torch.empty(n, 3, R, R, device=self.device)
        k.image_prep_ex(dev[head:], torch.from_numpy(d.copy()), dev[:head].view(torch.int64), pix, filter=0, mean=IMAGENET_MEAN,
                        std=IMAGENET_STD)
        x = torch.empty(n, R, R, 3, device=self.device)
        k.nchw_to_nhwc(pix, x, n, 3, R * R, 3)
        return x

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
