"""`InceptionV3FID`: pytorch-fid's `InceptionV3(output_blocks=[3])` on libpdmk - the feature extractor of clean-fid's
`legacy_pytorch` FID (pdm/utils/fid_utils.py).  fp32, inference only, NHWC; a `ConvTrunk` (pdm/models/convnet.py).

Every unit is one pdmk_conv2d_fwd launch (BatchNorm folded into weight and bias in float64 on the host, ReLU in the
epilogue); the 1x1 units go through the same kernel, so they get the fused ReLU and the column-slice output too.  A Mixed
block allocates its output [B * H * W, C_out] once and every branch's last unit writes its column slice of it (row stride
C_out): no concat copies.  Pools are pdmk_pool2d (the branch_pool average divides by the taps inside the image; Mixed_7c's
branch_pool is a max pool - the FID network's deviations from torchvision's), the head is pdmk_global_avgpool over the
8 x 8 map.
"""
import torch

from ... import _pdmk as k
from ..convnet import ConvTrunk, Map, checked, fold_unit, hub_checkpoint, load_weights_file
from . import spec as S

WEIGHTS_NAME = "pt_inception-2015-12-05-6726825d.pth"
INPUT_SIZE = 299
FEATURE_DIM = 2048


def default_weights_path():
    """Where torch hub keeps pytorch-fid's / clean-fid's Inception weights."""
    return hub_checkpoint(WEIGHTS_NAME)


class InceptionV3FID(ConvTrunk):
    def __init__(self, device=None, seed=0, init=True):
        super().__init__(device, S.build_units())
        if init:
            self.load_state_dict(S.init_state_dict(seed))

    @classmethod
    def from_pretrained(cls, path=None, device=None):
        """The weights file given, else torch hub's cache; never fetched."""
        sd = load_weights_file(path, WEIGHTS_NAME, "--inception_weights", "pytorch-fid Inception")
        model = cls(device=device, init=False)
        model.load_state_dict(sd)
        return model

    def load_state_dict(self, sd):
        """pytorch-fid's keys; fc.*, AuxLogits.* and num_batches_tracked are ignored, a missing / mis-shaped trunk key raises."""
        units = list(self.units.values())
        sd = checked(sd, S.state_dict_shapes(units, num_batches_tracked=False), "Inception", S.ignored)
        host = torch.zeros(self.arena.numel(), dtype=torch.float32)
        for u in units:
            self.fill_conv(host, u, *fold_unit(sd, *S.keys(u), S.BN_EPS))
        self.arena.copy_(host)

    # ------------------------------------------------------------------ ops
    def conv(self, x, name, out=None):
        """Every unit ends in a ReLU."""
        return super().conv(x, name, True, out=out)

    def _chain(self, x, names, out):
        for n in names[:-1]:
            x = self.conv(x, n)
        return self.conv(x, names[-1], out=out)

    def _mixed(self, x, n, widths, stride=1):
        """The block's output map and its column slices, one per entry of `widths`."""
        H, W = ((x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1) if stride == 2 else (x.H, x.W)
        y = self.new_map(x.B, H, W, sum(widths))
        cols, c = [], 0
        for wd in widths:
            cols.append(y.t[:, c:c + wd])
            c += wd
        return y, cols

    def _block_a(self, x, n):
        y, s = self._mixed(x, n, [64, 64, 96, self.units[f"{n}.branch_pool"].co])
        self.conv(x, f"{n}.branch1x1", out=s[0])
        self._chain(x, [f"{n}.branch5x5_1", f"{n}.branch5x5_2"], s[1])
        self._chain(x, [f"{n}.branch3x3dbl_1", f"{n}.branch3x3dbl_2", f"{n}.branch3x3dbl_3"], s[2])
        self.conv(self.pool(x, "avg", 1, 1), f"{n}.branch_pool", out=s[3])
        return y

    def _block_b(self, x, n):
        y, s = self._mixed(x, n, [384, 96, x.C], stride=2)
        self.conv(x, f"{n}.branch3x3", out=s[0])
        self._chain(x, [f"{n}.branch3x3dbl_1", f"{n}.branch3x3dbl_2", f"{n}.branch3x3dbl_3"], s[1])
        self.pool(x, "max", 2, 0, out=s[2])
        return y

    def _block_c(self, x, n):
        y, s = self._mixed(x, n, [192, 192, 192, 192])
        self.conv(x, f"{n}.branch1x1", out=s[0])
        self._chain(x, [f"{n}.branch7x7_{i}" for i in (1, 2, 3)], s[1])
        self._chain(x, [f"{n}.branch7x7dbl_{i}" for i in (1, 2, 3, 4, 5)], s[2])
        self.conv(self.pool(x, "avg", 1, 1), f"{n}.branch_pool", out=s[3])
        return y

    def _block_d(self, x, n):
        y, s = self._mixed(x, n, [320, 192, x.C], stride=2)
        self._chain(x, [f"{n}.branch3x3_1", f"{n}.branch3x3_2"], s[0])
        self._chain(x, [f"{n}.branch7x7x3_{i}" for i in (1, 2, 3, 4)], s[1])
        self.pool(x, "max", 2, 0, out=s[2])
        return y

    def _block_e(self, x, n, pool):
        y, s = self._mixed(x, n, [320, 384, 384, 384, 384, 192])
        self.conv(x, f"{n}.branch1x1", out=s[0])
        b = self.conv(x, f"{n}.branch3x3_1")
        self.conv(b, f"{n}.branch3x3_2a", out=s[1])
        self.conv(b, f"{n}.branch3x3_2b", out=s[2])
        b = self.conv(self.conv(x, f"{n}.branch3x3dbl_1"), f"{n}.branch3x3dbl_2")
        self.conv(b, f"{n}.branch3x3dbl_3a", out=s[3])
        self.conv(b, f"{n}.branch3x3dbl_3b", out=s[4])
        self.conv(self.pool(x, pool, 1, 1), f"{n}.branch_pool", out=s[5])
        return y

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward_nhwc(self, x):
        """x fp32 [B, 299, 299, 3] in [-1, 1] on the device -> pool3 features [B, 2048] fp32."""
        B, H, W, C = x.shape
        assert C == 3 and x.dtype == torch.float32 and x.is_contiguous() and min(H, W) >= 75, tuple(x.shape)
        m = Map(x.reshape(B * H * W, 3), B, H, W)
        for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            m = self.conv(m, n)
        m = self.pool(m, "max", 2, 0)
        m = self.conv(self.conv(m, "Conv2d_3b_1x1"), "Conv2d_4a_3x3")
        m = self.pool(m, "max", 2, 0)
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            m = self._block_a(m, n)
        m = self._block_b(m, "Mixed_6a")
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            m = self._block_c(m, n)
        m = self._block_d(m, "Mixed_7a")
        m = self._block_e(m, "Mixed_7b", "avg")
        m = self._block_e(m, "Mixed_7c", "max")
        out = torch.empty((B, m.C), device=self.device, dtype=torch.float32)
        k.global_avgpool(m.t, m.ld, out, B, m.H * m.W, m.C)
        return out

    @torch.no_grad()
    def features(self, images):
        """uint8 images -> [B, 2048] fp32: a list of [H, W, 3] arrays / tensors (any sizes) or one [B, H, W, 3] tensor,
        resized on the device (pdmk_resize_bilinear_u8) and run through the network."""
        from ...utils.fid_utils import pack_images, prep_images
        if torch.is_tensor(images) and images.dim() == 4:
            images = list(images.cpu())
        arrays = [torch.as_tensor(a).cpu().numpy() for a in images]
        packed, desc = pack_images(arrays)
        return self.forward_nhwc(prep_images(packed, desc, self.device))
