"""`AlexNetLPIPS` and `VGG19Style`: the two small trunks of the perceptual metrics on libpdmk, with their metric heads.
fp32, inference only, NHWC; `ConvTrunk`s (pdm/models/convnet.py): one weight arena, every conv one pdmk_conv2d_fwd launch
(exact-fp32 MFMA implicit GEMM), launches eager on the current stream, weights from files that are never fetched.

Both take a batch of PAIRS as one batch of 2 B images (the B originals, then the B edited ones), so a tap is one buffer whose two
halves are the two maps the head kernels compare:
* AlexNetLPIPS: ReLU fused into each conv, pdmk_pool2d (3 x 3, stride 2) behind the first two; each of the five post-ReLU maps
  goes through pdmk_lpips_layer, which adds the layer's distance to the fp64 result.
* VGG19Style: the taps are the PRE-ReLU outputs of conv_1 .. conv_5 (the reference inserts its loss modules straight behind the
  convs), so the convs run with relu = 0, pdmk_gram_pair reads the tap (style; conv_4 also content) and pdmk_relu_pool then
  feeds the next conv (in place where there is no pool).

The input normalisation is NOT folded into the first conv: zero padding applies to the normalised image, so a folded mean would
be wrong on the border pixels.  pdmk_image_prep_ex normalises ((x - mean) / std of the [0, 1] image; for LPIPS the composed
pair of spec.lpips_input_norm) and pdmk_nchw_to_nhwc lays the result out for the first conv.
"""
import torch

from ... import _pdmk as k
from ..convnet import ConvTrunk, Map, checked, load_weights_file
from . import spec as S


class _Trunk(ConvTrunk):
    """A trunk of conv + bias units under torchvision's `features.N.{weight,bias}`, run on a batch of pairs."""
    UNITS, WHAT = (), ""

    def __init__(self, device, extra=None):
        super().__init__(device, self.UNITS, extra)

    def _fill_convs(self, host, sd):
        sd = checked(sd, S.conv_shapes(self.UNITS), self.WHAT)
        for u in self.UNITS:
            self.fill_conv(host, u, sd[f"{u.name}.weight"], sd[f"{u.name}.bias"])

    def _input(self, x):
        B2, H, W, C = x.shape
        assert C == 3 and x.dtype == torch.float32 and x.is_contiguous() and B2 % 2 == 0, tuple(x.shape)
        return Map(x.reshape(B2 * H * W, 3), B2, H, W)

    @torch.no_grad()
    def prep(self, images_a, images_b, imsize):
        """Two equally long lists of SQUARE uint8 [H, W, 3] arrays -> the normalised fp32 NHWC batch [2 B, imsize, imsize, 3]:
        Pillow's bilinear Resize(imsize) + ToTensor bit for bit (pdmk_image_prep_ex, filter 0), then this trunk's Normalize."""
        from ...utils.clip_utils import pack_images
        from ...utils.data import prep_nhwc
        arrays = list(images_a) + list(images_b)
        assert len(images_a) == len(images_b) and arrays
        for a in arrays:
            if a.ndim != 3 or a.shape[2] != 3 or a.dtype.name != "uint8" or a.shape[0] != a.shape[1]:
                raise ValueError(f"expected square uint8 [H, W, 3] images, got {a.dtype} {a.shape}")
        packed, desc = pack_images(arrays, imsize)
        return prep_nhwc(packed, desc, imsize, self.device, 0, self.MEAN, self.STD)


class AlexNetLPIPS(_Trunk):
    """lpips.LPIPS(net='alex') (v0.1, spatial=False): distance of each pair of a batch."""
    UNITS, WHAT = S.ALEX_UNITS, "AlexNet"
    MEAN, STD = S.lpips_input_norm()

    def __init__(self, device=None, seed=0, init=True):
        super().__init__(device, {S.lin_key(i): c for i, c in enumerate(S.LPIPS_CHANNELS)})
        if init:
            self.load_state_dict(S.init_conv_state_dict(self.UNITS, seed), S.init_lin_state_dict(seed + 1))

    @classmethod
    def from_pretrained(cls, alexnet_weights=None, lpips_weights=None, device=None):
        """torchvision's AlexNet checkpoint and lpips' v0.1 linear heads from the files given, else torch hub's cache."""
        sd = load_weights_file(alexnet_weights, S.ALEX_WEIGHTS_NAME, "--alexnet_weights", "torchvision AlexNet")
        lin = load_weights_file(lpips_weights, S.LPIPS_WEIGHTS_NAME, "--lpips_weights", "lpips v0.1 (weights/v0.1/alex.pth)")
        model = cls(device=device, init=False)
        model.load_state_dict(sd, lin)
        return model

    def load_state_dict(self, sd, lin):
        """torchvision's `features.N.{weight,bias}` (classifier.* ignored) and lpips' `linN.model.1.weight`."""
        host = torch.zeros(self.arena.numel(), dtype=torch.float32)
        self._fill_convs(host, sd)
        for n, t in checked(lin, S.lin_shapes(), "lpips").items():
            host[self.offsets[n]:self.offsets[n] + t.numel()] = t.detach().reshape(-1).to(torch.float32)
        self.arena.copy_(host)

    @torch.no_grad()
    def forward_nhwc(self, x):
        """x fp32 [2 B, H, W, 3], scaled (prep): the B first images against the B last -> LPIPS fp64 [B] on the device."""
        m = self._input(x)
        B = m.B // 2
        out = torch.zeros(B, device=self.device, dtype=torch.float64)
        for i, u in enumerate(self.UNITS):
            m = self.conv(m, u, True)
            HW = m.H * m.W
            o = self.offsets[S.lin_key(i)]
            k.lpips_layer(m.t, m.t[B * HW:], m.ld, self.arena[o:o + u.co], out, B, HW, u.co)
            if i in S.ALEX_POOL_AFTER:
                m = self.pool(m, "max", 2, 0)
        return out


class VGG19Style(_Trunk):
    """styleloss.py's get_style_content_loss with the original as style and content image: per pair (style, content, total)."""
    UNITS, WHAT = S.VGG_UNITS, "VGG-19"
    MEAN, STD = S.IMAGENET_MEAN, S.IMAGENET_STD

    def __init__(self, device=None, seed=0, init=True):
        super().__init__(device)
        if init:
            self.load_state_dict(S.init_conv_state_dict(self.UNITS, seed))

    @classmethod
    def from_pretrained(cls, vgg_weights=None, device=None):
        sd = load_weights_file(vgg_weights, S.VGG_WEIGHTS_NAME, "--vgg_weights", "torchvision VGG-19")
        model = cls(device=device, init=False)
        model.load_state_dict(sd)
        return model

    def load_state_dict(self, sd):
        """torchvision's `features.N.{weight,bias}`; the layers behind conv_5 and classifier.* are ignored."""
        host = torch.zeros(self.arena.numel(), dtype=torch.float32)
        self._fill_convs(host, sd)
        self.arena.copy_(host)

    @torch.no_grad()
    def forward_nhwc(self, x):
        """x fp32 [2 B, H, W, 3], ImageNet-normalised (prep) -> (style, content, total), each fp64 [B] on the device."""
        m = self._input(x)
        B = m.B // 2
        style = torch.zeros(B, device=self.device, dtype=torch.float64)
        content = torch.zeros(B, device=self.device, dtype=torch.float64)
        for i, u in enumerate(self.UNITS):
            m = self.conv(m, u, False)
            HW = m.H * m.W
            ws = torch.empty(k.gram_workspace_elems(B, HW, m.C), device=self.device, dtype=torch.float32)
            k.gram_pair(m.t, m.t[B * HW:], m.ld, B, HW, m.C, ws, style, content if i == S.VGG_CONTENT else None)
            if i == len(self.UNITS) - 1:
                break
            if i in S.VGG_POOL_AFTER:
                if min(m.H, m.W) < 2:
                    raise ValueError(f"VGG19Style: a {m.H} x {m.W} map is too small for the 2 x 2 max pool")
                y = self.new_map(m.B, m.H // 2, m.W // 2, m.C)
                k.relu_pool(m.t, m.ld, y.t, y.ld, m.B, m.H, m.W, m.C, 2)
                m = y
            else:
                k.relu_pool(m.t, m.ld, m.t, m.ld, m.B, m.H, m.W, m.C, 0)      # elementwise: in place
        return style, content, S.STYLE_WEIGHT * style + S.CONTENT_WEIGHT * content
