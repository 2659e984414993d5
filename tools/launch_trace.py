#!/usr/bin/env python3
"""Fingerprint of the library-call sequence of the host side: the check that a refactor of the Python above libpdmk did not
change what is launched.  Every function of `_pdmk._SIGS` is wrapped on `_pdmk._lib`; a call is recorded as its name, every
non-pointer argument, and for a pointer only whether it is null (pdmk_gemm_args: the same rule over the struct's fields, for
every problem of a grouped launch).  Tiny scenarios, per scenario the call count and a sha256 of the record:
  unet-f32 / unet-bf16  tests/dp_worker.py's recipe: tiny U-Net, arch vector 0.55, B = 2, 16x16 latent, 13x64 text; one eager
                        main step + AdamW, one upper step + its AdamW
  vae-bf16              the tiny VAE of tests/test_vae_gpu.py: encode_latents, decode
  clip-text-bf16        the tiny CLIPTextModel of tests/test_clip_gpu.py, one call
  clip-model-f32        the tiny CLIPModel of tests/test_clip_model_gpu.py: encode_image, encode_text
  sample-pndm-f32 /     StableDiffusionPruningPipeline over a seeded tiny U-Net (budget 0.6) and VAE: B = 1, 16x16 latent, 13x64
  sample-ddim-f32       text embeddings, 4 steps, guidance 7.5, the eager loop, latents out - every scheduler step's pdmk_axpby
                        coefficients are in the record
  inception-f32         InceptionV3FID(seed=0): forward_nhwc on a seeded [2, 75, 75, 3] input, features on 40x40 and 50x37 images
  resnet-f32            ResNet50Classifier(seed=0, layers=(1, 1, 1, 1)): classify 40x40, 50x37, 37x50 at resize 36, crop 32, batch 2
  lpips-f32 / vgg-f32   AlexNetLPIPS(seed=0) on two 64-px pairs, VGG19Style(seed=0) on two 37-px pairs: prep + forward_nhwc
  clip-prep             clip_utils.pack_images + prep_images at R = 48 on 37x53, 64x64 and 300x200 images
  data-to_device        one PackedBatches batch of three in-memory rows through data.to_device
The call record does not see behind pointers, so these six also print a sha256 over tensors: the model's weight arena, every
packed image batch as the prep kernel is handed it (image bytes and both descriptor copies; the alignment bytes between
images are masked to zero first, because a loader that leaves them uninitialised is still the same launch) and every result.
GEMM plans come from the untuned decision tree and the CLIP towers run eagerly (PDMK_GEMM_TUNE=0, PDMK_CLIP_GRAPH=0, set
here), so two runs of one commit print the same digests.  It touches only `_pdmk` and the public model classes: the same file
runs on an older checkout.  What the digest does not see: anything behind a pointer other than pdmk_gemm_args - the
POINTER(c_int32) outputs and the item arrays of pdmk_reduce_partials_group / pdmk_splitk_finish_group are recorded as null or
not, so WHAT a deferred queue flushes is covered only by its item count.
    python tools/launch_trace.py [--dump DIR]   (DIR/<scenario>.txt: one call per line)"""
import argparse
import ctypes as C
import hashlib
import os
import sys

os.environ["PDMK_GEMM_TUNE"] = "0"
os.environ["PDMK_CLIP_GRAPH"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "unlearn-ft_amd"), os.path.join(ROOT, "oracle")]
import torch  # noqa: E402
from pdm import _pdmk as k  # noqa: E402

CALLS = []
DATA = []           # tensors of the current scenario for the second digest
GEMM_P = C.POINTER(k.GemmArgs)


def _null(a):
    return not (a.value if isinstance(a, C.c_void_p) else a)


def _struct(g):
    return tuple(_null(getattr(g, n)) if t is C.c_void_p else getattr(g, n) for n, t in k.GemmArgs._fields_)


def _arg(tp, a):
    if tp is GEMM_P:          # byref(one argument block), or the array of a grouped launch
        return tuple(_struct(g) for g in a) if isinstance(a, C.Array) else _struct(a._obj)
    if tp is C.c_void_p or issubclass(tp, C._Pointer):
        return _null(a)
    return getattr(a, "value", a)


def _wrap(name, fn, argtypes):
    def call(*args):
        CALLS.append((name,) + tuple(_arg(t, a) for t, a in zip(argtypes, args)))
        return fn(*args)
    return call


for _n, (_a, _r) in k._SIGS.items():
    setattr(k._lib, _n, _wrap(_n, getattr(k._lib, _n), _a))


def unet(dtype):
    from pdm_ref import arch as oarch, weights as oweights
    from pdm_ref.config import UNetConfig as OCfg
    from pdm.models.unet.spec import UNetConfig
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    from pdm.training.bilevel import BilevelStepper
    dense = oweights.init_dense_state_dict(OCfg.tiny(), seed=0)
    av = oarch.random_arch_vector(OCfg.tiny(), 0.55, seed=0, drop_depth=(1, 9))
    student = UNet2DConditionModelPruned(UNetConfig.tiny(), av, "cuda:0", dtype, train=True, init=False)
    teacher = UNet2DConditionModelPruned(UNetConfig.tiny(), None, "cuda:0", dtype, train=False, init=False)
    student.load_dense_or_pruned(dense)
    teacher.load_dense_or_pruned(dense)
    st = BilevelStepper(student, teacher, lr=1e-4, upper_lr=2e-4, bilevel=True, bucket_mb=1)
    g = torch.Generator().manual_seed(97)
    lat, noise = torch.randn(2, 4, 16, 16, generator=g).cuda(), torch.randn(2, 4, 16, 16, generator=g).cuda()
    t, ehs = torch.randint(0, 1000, (2,), generator=g).cuda(), torch.randn(2, 13, 64, generator=g).cuda()
    empty = torch.randn(1, 13, 64, generator=g).expand(2, 13, 64).contiguous().cuda()
    st.main_step(lat, noise, t, ehs)
    st.optimizer_step(upper=False)
    st.upper_step(lat, noise, t, ehs, empty)
    st.optimizer_step(upper=True)


def vae():
    from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
    m = AutoencoderKL(VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1), "cuda:0", torch.bfloat16, seed=7)
    g = torch.Generator().manual_seed(1)
    m.encode_latents((torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).cuda(), noise=torch.randn(2, 4, 8, 8, generator=g).cuda())
    m.decode(torch.randn(2, 4, 8, 8, generator=g).cuda())


TEXT = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2)


def _ids():
    ids = torch.randint(0, 998, (2, 77), generator=torch.Generator().manual_seed(2))
    ids[:, 0], ids[0, 20], ids[1, 61] = 998, 999, 999          # begin-of-text; end-of-text = the largest id of its row
    return ids


def clip_text():
    from pdm.models.clip.text_encoder import CLIPTextConfig, CLIPTextModel
    CLIPTextModel(CLIPTextConfig(**TEXT), "cuda:0", torch.bfloat16, seed=5)(_ids())


def clip_model():
    from pdm.models.clip.clip_model import CLIPModel
    vision = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=224, patch_size=32)
    m = CLIPModel.from_configs(dict(TEXT, hidden_act="quick_gelu"), vision, 64, device="cuda:0", dtype=torch.float32, seed=11)
    m.encode_image(torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(3)))
    m.encode_text(_ids())


def sample(scheduler):
    from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
    from pdm.pipelines import pruning_pipelines as P
    cfg = UNetConfig.tiny()
    unet = UNet2DConditionModelPruned(cfg, arch_vector_for_budget(cfg, 0.6, hw=16)[0], "cuda:0", torch.float32, train=False, seed=3)
    vae = AutoencoderKL(VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1), "cuda:0", torch.float32, seed=7)
    pipe = P.StableDiffusionPruningPipeline(vae, None, unet, getattr(P, scheduler)(prediction_type="v_prediction"))
    g = torch.Generator().manual_seed(4)
    pe, ne, lat = torch.randn(1, 13, 64, generator=g), torch.randn(1, 13, 64, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    pipe(prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(), latents=lat.cuda(), num_inference_steps=4, guidance_scale=7.5,
         graph=False, output_type="latent")


# ---- the evaluation nets: what is behind the pointers (weight arena, packed image batch, results) goes into a second digest
def _prep_seen(fn):
    """A pdm._pdmk image-prep entry point that also puts its packed batch into DATA: the image bytes as the device holds
    them (the up-to-3 alignment bytes behind each image masked to zero) and both copies of the descriptors."""
    def call(src, desc, desc_dev, *args, **kw):
        img = src.cpu().clone()
        for off, h, w in desc[:, :3].tolist():
            img[off + h * w * 3:(off + h * w * 3 + 3) & ~3] = 0
        DATA.extend([img, desc, desc_dev])
        return fn(src, desc, desc_dev, *args, **kw)
    return call


for _n in ("image_prep", "image_prep_ex", "resize_bilinear_u8"):
    setattr(k, _n, _prep_seen(getattr(k, _n)))


def _images(seed, sizes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy() for h, w in sizes]


def inception():
    from pdm.models.inception.inception_v3 import InceptionV3FID
    m = InceptionV3FID(seed=0)
    x = torch.rand(2, 75, 75, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1
    DATA.extend([m.arena, m.forward_nhwc(x.cuda()), m.features(_images(6, [(40, 40), (50, 37)]))])


def resnet():
    from pdm.models.resnet import ResNet50Classifier
    m = ResNet50Classifier(seed=0, layers=(1, 1, 1, 1))
    DATA.extend([m.arena, *m.classify(_images(7, [(40, 40), (50, 37), (37, 50)]), resize_size=36, crop_size=32, batch_size=2)])


def perceptual(cls, px):
    from pdm.models import perceptual as P
    m = getattr(P, cls)(seed=0)
    out = m.forward_nhwc(m.prep(_images(8, [(px, px)] * 2), _images(9, [(px, px)] * 2), px))
    DATA.extend([m.arena, *(out if isinstance(out, tuple) else (out,))])


def clip_prep():
    from pdm.utils import clip_utils
    packed, desc = clip_utils.pack_images(_images(10, [(37, 53), (64, 64), (300, 200)]), 48)
    DATA.extend([packed, desc, clip_utils.prep_images(packed, desc, 48, "cuda:0")])


def data_to_device():
    """Three in-memory rows (3, 0 and 1 bytes mod 4) as one training batch: random crop and flip at 32 px, no tokenizer."""
    from PIL import Image
    from pdm.utils import data as D
    rows = [{"image": Image.fromarray(a), "caption": f"row {i}"} for i, a in enumerate(_images(11, [(37, 53), (40, 41), (33, 35)]))]
    ds = D.PackedBatches(rows, resolution=32, tokenizer=None, image_column="image", caption_column="caption", train=True,
                         center_crop=False, random_flip=True, seed=0, rank=0)
    ds.plan = [[0, 1, 2]]
    out = D.to_device(ds[0], 32, "cuda:0")
    DATA.extend([out["image_desc"], out["index"], out["pixel_values"]])


def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(f"{t.dtype} {tuple(t.shape)} ".encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", help="directory for one text file per scenario, one call per line")
    a = ap.parse_args()
    for name, fn in (("unet-f32", lambda: unet(torch.float32)), ("unet-bf16", lambda: unet(torch.bfloat16)), ("vae-bf16", vae),
                     ("clip-text-bf16", clip_text), ("clip-model-f32", clip_model),
                     ("sample-pndm-f32", lambda: sample("PNDMScheduler")), ("sample-ddim-f32", lambda: sample("DDIMScheduler")),
                     ("inception-f32", inception), ("resnet-f32", resnet), ("lpips-f32", lambda: perceptual("AlexNetLPIPS", 64)),
                     ("vgg-f32", lambda: perceptual("VGG19Style", 37)), ("clip-prep", clip_prep),
                     ("data-to_device", data_to_device)):
        del CALLS[:], DATA[:]
        fn()
        torch.cuda.synchronize()
        lines = [repr(c) for c in CALLS]
        print(f"{name:16s} calls {len(lines):6d}  sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}"
              + (f"  tensors {len(DATA):3d}  sha256 {_digest(DATA)}" if DATA else ""), flush=True)
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            with open(os.path.join(a.dump, name + ".txt"), "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
