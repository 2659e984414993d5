"""ConceptPrune's neuron removal, host side (no GPU): the bit layout helpers against a Python loop, the table of
pdmk_masked_weights, the slot of a U-Net call, the result path, remove_neurons.py's flags and its errors."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import neuron_removal_fixtures as nf
from pdm.utils import concept_prune as CP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name="remove_neurons"):
    spec = importlib.util.spec_from_file_location(name + "_nr_host", os.path.join(ROOT, "unlearn-ft_amd", "scripts", "baselines",
                                                                                 "concept_prune", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the bit layout
@pytest.mark.parametrize("Fd", [8, 72, 1000, 5120])
def test_pack_and_unpack_against_a_loop(Fd):
    g = torch.Generator().manual_seed(Fd)
    mask = torch.rand(3, Fd, generator=g) < 0.4
    mask[0, Fd - 1] = True                                    # the last column, and bit 31 of a word where there is one
    if Fd > 31:
        mask[1, 31] = True
    words = CP.pack_bits(mask)
    rw = (Fd + 31) // 32
    assert words.dtype == torch.int32 and tuple(words.shape) == (3, rw)
    assert torch.equal(words, nf.pack_loop(mask))
    assert torch.equal(CP.unpack_bits(words, Fd), mask) and torch.equal(nf.unpack_loop(words, Fd), mask)
    if Fd % 32:                                               # the bits past F are 0, and unpack does not read them
        assert int(words[0, -1]) >> (Fd % 32) == 0
        dirty = words.clone()
        dirty[:, -1] |= torch.tensor(-(1 << (Fd % 32)), dtype=torch.int32)
        assert torch.equal(CP.unpack_bits(dirty, Fd), mask)
    # leading dimensions
    m3 = torch.stack([mask, ~mask])
    assert torch.equal(CP.unpack_bits(CP.pack_bits(m3), Fd), m3) and tuple(CP.pack_bits(m3).shape) == (2, 3, rw)
    with pytest.raises(ValueError):
        CP.unpack_bits(words, Fd + 32)


def test_mask_table_layout():
    from pdm import _pdmk as k
    assert [k.mask_row_words(Fd) for Fd in (1, 8, 32, 33, 72, 1000, 5120)] == [1, 1, 1, 2, 3, 32, 160]
    placed = [(16, 5, 8, 8), (96, 40, 72, 96), (4000, 17, 2568, 2568)]
    t = k.MaskTable(placed, "cpu")
    assert t.layers == [(16, 0, 0, 5, 8, 8), (96, 40, 5, 40, 72, 96), (4000, 40 + 3840, 5 + 120, 17, 2568, 2568)]
    assert (t.extent, t.src_elems, t.words) == (4000 + 17 * 2568, 40 + 3840 + 43656, 5 + 120 + 17 * 81)
    rec = np.dtype([("dst", "<i8"), ("src", "<i8"), ("bits", "<i8"), ("O", "<i4"), ("F", "<i4"), ("ld", "<i4"), ("pad", "<i4")])
    rows = np.frombuffer(t.dev.numpy().tobytes(), dtype=rec)
    assert rec.itemsize == 40 and len(rows) == t.nrows == 1 + 1 + 3          # 6 rows of 2568 columns per workgroup
    assert rows["O"].tolist() == [5, 40, 6, 6, 5] and rows["F"].tolist() == [8, 72, 2568, 2568, 2568]
    assert rows["dst"].tolist() == [16, 96, 4000, 4000 + 6 * 2568, 4000 + 12 * 2568]
    assert rows["src"].tolist() == [0, 40, 3880, 3880 + 6 * 2568, 3880 + 12 * 2568]
    assert rows["bits"].tolist() == [0, 5, 125, 125 + 6 * 81, 125 + 12 * 81]
    # every weight row of every layer is in exactly one block
    for (d, O, Fd, ld) in placed:
        mine = rows[(rows["F"] == Fd)]
        assert sorted((int(r["dst"]) - d) // ld + o for r in mine for o in range(int(r["O"]))) == list(range(O))
    for bad in ([], [(0, 0, 8, 8)], [(0, 4, 8, 7)], [(-8, 4, 8, 8)]):
        with pytest.raises(k.PdmkError):
            k.MaskTable(bad, "cpu")


# ---- slots
def test_slot_of_a_call():
    assert [CP.call_slot(c) for c in range(4)] == [0, 1, 2, 3]                          # DDIM: one call per step
    assert [CP.call_slot(c, repeat_first=True) for c in range(5)] == [0, 0, 1, 2, 3]    # PNDM: the first timestep twice
    obs = SimpleNamespace(call=0, repeat_first=True)                                    # WandaObserver.slot is the same rule
    for c in range(5):
        obs.call = c
        assert CP.WandaObserver.slot(obs) == CP.call_slot(c, True)
        obs.repeat_first = False
        assert CP.WandaObserver.slot(obs) == CP.call_slot(c)
        obs.repeat_first = True


# ---- paths, flags, errors
def test_after_removal_path():
    a = SimpleNamespace(hook_module="unet", seed=43, res_path="results/stable-diffusion", result_dir=None,
                        model_id="stabilityai/stable-diffusion-2-1", target="Van Gogh", skill_ratio=0.01)
    res = "results/results_seed_43/stable-diffusion/stabilityai/stable-diffusion-2-1/Van Gogh"
    assert CP.result_paths(a).after_removal_results == res + "/after_removal_results/0.01"
    a.result_dir, a.skill_ratio = "/r", 0.25
    assert CP.result_paths(a).after_removal_results == "/r/stabilityai/stable-diffusion-2-1/Van Gogh/after_removal_results/0.25"


def test_flags_and_settings():
    rn = _script()
    a = rn.parse_args(["--target", "Monet", "--ckpt_path", "/a/b/"])
    assert all(getattr(a, n) is None for n in ("gpu", "dbg", "base", "model_id", "skill_ratio", "target_file", "timesteps",
                                               "base_config_path", "hook_module", "seed", "result_dir", "mixed_precision"))
    assert a.scheduler == "ddim"
    a = CP.resolve_args(a)
    assert (a.gpu, a.base, a.skill_ratio, a.timesteps, a.hook_module, a.seed, a.res_path, a.model_id) == \
           (0, "things", 0.01, 50, "unet", 43, "results/stable-diffusion", "stabilityai/stable-diffusion-2-1")
    a = CP.resolve_args(rn.parse_args(["--target", "naked", "--ckpt_path", "/a/", "--skill_ratio", "0.02", "--gpu", "1",
                                       "--dbg", "1", "--base", "things", "--model_id", "m", "--target_file", "f.txt"]))
    assert (a.skill_ratio, a.gpu, a.dbg, a.model_id, a.target_file, a.timesteps) == (0.02, 1, True, "m", "f.txt", 50)
    assert (rn.CANVAS, rn.TILE, rn.LEFT, rn.RIGHT) == ((530, 290), (256, 256), (0, 40), (275, 40))
    assert (rn.PROMPT_AT, rn.LABEL_AT, rn.LABEL) == ((80, 15), (350, 15), "w/o skilled neurons")


def test_canvas():
    rn = _script()
    plain = np.full((64, 64, 3), 200, dtype=np.uint8)
    removed = np.full((48, 48, 3), 90, dtype=np.uint8)
    im = rn.compose(plain, removed, "a cat in the style of Monet")
    assert im.size == (530, 290) and im.mode == "RGB"
    px = np.asarray(im)
    assert (px[40:296, 0:256] == 200).all() and (px[40:296, 275:531] == 90).all()      # both resized to 256 x 256, pasted
    assert (px[40:, 256:275] == 0).all() and (px[:10] == 0).all()
    assert (px[15:35, 80:256] > 0).any() and (px[15:35, 350:500] > 0).any()            # the two captions
    assert (px[10:40, :80] == 0).all()                                                 # and nothing in front of the first


def test_missing_norms_name_wanda(tmp_path):
    """Raised from the result directory alone: no model is loaded and no device is asked for."""
    argv = ["--target", "Monet", "--ckpt_path", "/a/b/", "--result_dir", str(tmp_path / "r"), "--model_id", "snap"]
    with pytest.raises(FileNotFoundError, match=r"base_norms\.pt.*wanda\.py"):
        _script().main(argv)
    res = tmp_path / "r" / "snap" / "Monet"
    res.mkdir(parents=True)
    torch.save({}, res / "base_norms.pt")
    with pytest.raises(FileNotFoundError, match=r"target_norms\.pt.*wanda\.py"):
        _script().main(argv)
    assert not (res / "after_removal_results").exists()
    with pytest.raises(NotImplementedError, match="target_file"):
        _script().main(argv + ["--target_file", "x.txt"])


@pytest.mark.parametrize("hook", ["text", "unet-ffn-1", "attn_key", "attn_val"])
def test_unbuilt_hook_modules_raise(hook, tmp_path):
    with pytest.raises(NotImplementedError, match=hook):
        _script().main(["--target", "Monet", "--ckpt_path", "/a/b/", "--hook_module", hook, "--result_dir", str(tmp_path / "r")])
    assert not (tmp_path / "r").exists()
