"""The parameter-arena layout of every model, pinned: a sha256 over (key, kind, shape, srcs, logical, off) of every entry.
Checkpoints, optimiser state and the kernels' weight views all index the arenas by these offsets, so a refactor of the
`build_entries` functions must leave them bit-identical.  The constants were computed on the commit before
`assign_offsets` / `norm_pair` / `lin_pair` existed (each builder still had its own offset loop), not on the code under test."""
import hashlib

import pytest

from pdm_ref import arch as oarch
from pdm_ref.config import UNetConfig as OCfg


def digest(entries):
    h = hashlib.sha256()
    for e in entries:
        h.update(repr((e.key, e.kind, tuple(e.shape), [tuple(s) for s in e.srcs], tuple(e.logical), e.off)).encode())
    return h.hexdigest()


def _unet(pruned):
    from pdm.models.unet import params, spec
    cfg = spec.UNetConfig.tiny()
    av = oarch.random_arch_vector(OCfg.tiny(), 0.55, seed=0, drop_depth=(1, 9)) if pruned else None
    return params.build_entries(cfg, spec.apply_arch_vector(cfg, av))


def _vae(decoder):
    from pdm.models.vae.autoencoder_kl import VAEConfig, build_entries
    return build_entries(VAEConfig.sd21(), decoder)


def _text(proj):
    from pdm.models.clip.text_encoder import CLIPTextConfig, build_entries
    return build_entries(CLIPTextConfig.sd21(), proj)


def _vision(proj):
    from pdm.models.clip.clip_model import CLIPVisionConfig, build_vision_entries
    return build_vision_entries(CLIPVisionConfig(), proj)


PINNED = [
    ("unet-tiny-dense", _unet, False, 581, "5d3ba84e73961252dbda46866e0c2a28e2ec1729aa60ef23422c46ee91bacf01"),
    ("unet-tiny-pruned", _unet, True, 537, "0851a6774025ce6c712fcef37ca744c010c546b83120fd2b8210b757d06cb2e6"),
    ("vae-sd21", _vae, True, 244, "f0c4f944937d5f31d9f538a3c195f6e6d4ff5ac8b0b07c18c93cd30825b63b9f"),
    ("vae-sd21-encoder", _vae, False, 106, "b6c91dfa29a88993500b25e0c6661a8eee9561c06b2c4037cc17d035e41bcdbb"),
    ("clip-text-sd21", _text, 0, 280, "bec3541be41c65d7a3f76eb85ecf1266e637350fda333c2a0b58e75cb7fd38e9"),
    ("clip-text-sd21-proj512", _text, 512, 281, "238c1f2f4c5e35a9671cbb431c2bd466652e160658f4bb498b9a2e6e41fcac83"),
    ("clip-vision", _vision, 0, 151, "4a7162dbd39e710828bcd43719750dcd2bc32bc81f4a93928268c51e48d44bfe"),
    ("clip-vision-proj512", _vision, 512, 152, "8a4586b016455df325b8a0dbf528c1685e254ca8bdb7434d2ac1456fb2a35f18"),
]


@pytest.mark.parametrize("name,make,arg,count,want", PINNED, ids=[p[0] for p in PINNED])
def test_arena_layout_is_pinned(name, make, arg, count, want):
    entries = make(arg)
    assert len(entries) == count
    assert digest(entries) == want
