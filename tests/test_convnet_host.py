"""Host side of pdm/models/convnet.py (no GPU): the weight arenas of the four evaluation networks against the layout rule
written out here - per unit the weight [Co, kh * kw * Ci] then the bias [Co], further vectors behind them, each rounded up to
128 floats (a 512-byte line) - and against the sizes it gave when the networks were written."""
import pytest

from pdm.models import convnet
from pdm.models.inception import spec as inception
from pdm.models.perceptual import spec as perceptual
from pdm.models.resnet import spec as resnet

LIN = {perceptual.lin_key(i): c for i, c in enumerate(perceptual.LPIPS_CHANNELS)}
NETS = {      # what each model hands to ConvTrunk: (units, extra vectors), and the arena's size in floats
    "inception": (inception.build_units(), None, 21_773_440),
    "resnet50": (resnet.build_units() + [resnet.FC], None, 25_531_008),
    "resnet-tiny": (resnet.build_units((1, 1, 1, 1)) + [resnet.FC], None, 10_055_552),
    "alexnet": (list(perceptual.ALEX_UNITS), LIN, 2_471_168),
    "vgg19": (list(perceptual.VGG_UNITS), None, 555_520),
}


def _expected(units, extra):
    off, out = 0, {}
    for u in units:
        w = off
        off += (u.co * u.kh * u.kw * u.ci + 127) // 128 * 128
        out[u.name] = (w, off)
        off += (u.co + 127) // 128 * 128
    for name, n in (extra or {}).items():
        out[name] = off
        off += (n + 127) // 128 * 128
    return out, off


@pytest.mark.parametrize("net", sorted(NETS))
def test_arena_offsets(net):
    units, extra, total = NETS[net]
    offsets, size = convnet.arena_layout(units, extra)
    want, want_size = _expected(units, extra)
    assert size == want_size == total
    assert offsets == want and list(offsets) == [u.name for u in units] + list(extra or {})
    assert offsets[units[0].name][0] == 0
    last = units[-1]
    assert offsets[last.name][1] + (last.co + 127) // 128 * 128 == size - sum((n + 127) // 128 * 128 for n in (extra or {}).values())
    assert all(o % 128 == 0 for v in offsets.values() for o in (v if isinstance(v, tuple) else (v,)))


def test_arena_offsets_of_named_entries():
    off, _ = convnet.arena_layout(*NETS["inception"][:2])
    assert off["Conv2d_1a_3x3"] == (0, 896) and off["Conv2d_2a_3x3"] == (1024, 1024 + 9216)
    assert off["Mixed_7c.branch_pool"] == (21_773_440 - 256 - 2048 * 192, 21_773_440 - 256)
    off, size = convnet.arena_layout(*NETS["resnet50"][:2])
    assert off["conv1"] == (0, 9472) and off["fc"] == (size - 1024 - 2_048_000, size - 1024)
    assert off["layer4.2.conv3"][1] + 2048 == off["fc"][0]
    off, size = convnet.arena_layout(*NETS["alexnet"][:2])
    assert off["features.0"] == (0, 23_296)                              # 64 * 363 = 23 232 -> 23 296
    assert [off[n] for n in LIN] == [size - 1280, size - 1152, size - 896, size - 512, size - 256]
    off, size = convnet.arena_layout(*NETS["vgg19"][:2])
    assert off["features.0"] == (0, 1792) and off["features.10"] == (size - 256 - 294_912, size - 256)
