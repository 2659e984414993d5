"""UCE, host side (no GPU): slice indices from hand-worked token counts, the text-list builders, the preserve_scale default,
checkpoint names worked out by hand from the reference's rules, the golden artist list, the script's flags."""
import importlib.util
import os

import pytest

import uce_fixtures as fx
from pdm.utils import erasure_utils as E
from pdm.utils import uce as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARTISTS = ["Ada Alpha", "Bo Beta", "Cy Gamma", "Di Delta", "Ed Epsilon", "Van Gogh"]


def _script():
    spec = importlib.util.spec_from_file_location("train_erase_uce_host", os.path.join(
        ROOT, "unlearn-ft_amd", "scripts", "baselines", "unified_concept_editing", "train_erase.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- slices (n = BOS + words + EOS; 77-token rows)
@pytest.mark.parametrize("n_old,n_new,old,new", [
    (4, 4, (2, 77), (2, 77)),            # equal lengths: from the last word to the end, 75 rows
    (6, 3, (4, 77), (1, 74)),            # old longer: the new text loses its last three padding rows, 73 rows
    (3, 7, (1, 73), (5, 77)),            # new longer
    (5, 2, (3, 77), (0, 74)),            # ' ' is BOS + EOS: its slice starts at BOS
    (77, 4, (75, 77), (2, 4)),           # a truncated 77-token text: its last word and EOS, two rows
])
def test_pair_slices(n_old, n_new, old, new):
    assert U.pair_slices(n_old, n_new, 77) == (old, new)
    assert old[1] - old[0] == new[1] - new[0] == 77 - max(n_old, n_new) + 2
    so, sn = fx.slices(n_old, n_new, 77)                                # the oracle's own arithmetic agrees
    assert (so.start, so.stop, sn.start, sn.stop) == old + new


# ---- texts
def test_texts_art_plain_and_with_prompts():
    concepts, old, new, retain, _ = U.build_texts("Van Gogh", "art", artists=ARTISTS)
    assert concepts == ["Van Gogh"] and old == ["Van Gogh"] and new == [" "]
    assert retain == [""] + ARTISTS[:5]                                  # every artist but the erased one (case-insensitive)
    concepts, old, new, retain, _ = U.build_texts(" van gogh , Bo Beta", "art", guided_concepts="art", add_prompts=True,
                                                  artists=ARTISTS)
    assert concepts == ["van gogh", "Bo Beta"]
    assert old == ["van gogh", "painting by van gogh", "art by van gogh", "artwork by van gogh", "picture by van gogh",
                   "style of van gogh", "Bo Beta", "painting by Bo Beta", "art by Bo Beta", "artwork by Bo Beta",
                   "picture by Bo Beta", "style of Bo Beta"]
    assert new == ["art"] * 12
    assert retain == ["", "Ada Alpha", "Cy Gamma", "Di Delta", "Ed Epsilon"]


def test_texts_object_and_other():
    _, old, new, retain, _ = U.build_texts("church", "object", add_prompts=True)
    assert old == ["church", "image of church", "photo of church", "portrait of church", "picture of church", "painting of church"]
    assert new == [" "] * 6 and retain == [""]
    _, old, _new, retain, _ = U.build_texts("nudity", "unsafe", add_prompts=True)          # no templates for other types
    assert old == ["nudity"] and retain == [""]
    _, _old, _new, retain, _ = U.build_texts("church", "object", preserve_concepts="dog, a cat")
    assert retain == ["", "dog", "a cat"]


def test_texts_several_guided_concepts():
    _, old, new, _r, _ = U.build_texts("a, b", "object", guided_concepts="x, y", add_prompts=True)
    assert len(old) == 12 and new == ["x"] * 6 + ["y"] * 6
    _, old, new, _r, _ = U.build_texts("a, b", "other", guided_concepts="x, y")
    assert old == ["a", "b"] and new == ["x", "y"]
    with pytest.raises(ValueError):
        U.build_texts("a, b, c", "other", guided_concepts="x, y")


def test_sampled_artists_are_reproducible():
    all_artists = U.read_artists()
    a = U.build_texts("5artists", "art", preserve_number=7, seed=3)
    b = U.build_texts("5artists", "art", preserve_number=7, seed=3)
    c = U.build_texts("5artists", "art", preserve_number=7, seed=4)
    assert a == b and a[0] != c[0]
    concepts, old, _new, retain, name = a
    assert len(concepts) == 5 and old == concepts and set(concepts) <= set(all_artists)
    assert len(retain) == 8 and retain[0] == "" and not set(retain[1:]) & set(concepts)
    assert name == "5artists-towards_uncond-preserving_7artists-preserve_true-sd_2_1-method_replace"
    _, _, _, retain, _ = U.build_texts("Van Gogh", "art")                 # the list spells him "Vincent Van Gogh": all are kept
    assert retain == [""] + all_artists
    _, _, _, retain, _ = U.build_texts("vincent van gogh", "art")         # compared in lower case
    assert len(retain) == 1734 and "Vincent Van Gogh" not in retain and retain[:2] == ["", "A.J.Casson"]


@pytest.mark.parametrize("name", ["allartist", "i2g", "10artists", "imagenette"])
def test_fixed_lists_raise(name):
    with pytest.raises(NotImplementedError, match=name):
        U.build_texts(name, "art")


def test_base_and_technique():
    with pytest.raises(NotImplementedError):
        U.build_texts("x", "other", base="1.4")
    with pytest.raises(ValueError):
        U.build_texts("x", "other", technique="erase")


def test_preserve_scale_default():
    assert U.default_preserve_scale(None, [""]) == 1.0
    assert U.default_preserve_scale(None, [""] * 4) == 0.25
    assert U.default_preserve_scale(None, [""] * 1734) == 0.1
    assert U.default_preserve_scale(0.3, [""] * 1734) == 0.3


# ---- names (print_text)
@pytest.mark.parametrize("kw,name", [
    (dict(concepts="Van Gogh", concept_type="art", guided_concepts="art"),
     "van gogh-towards_art-preserve_true-sd_2_1-method_replace"),
    (dict(concepts="Van Gogh, Monet", concept_type="art", technique="tensor", preserve_number=3),
     "van gogh_monet-towards_uncond-preserving_3artists-preserve_true-sd_2_1-method_tensor"),
    (dict(concepts="Church", concept_type="object"), "church-towards_uncond-preserve_false-sd_2_1-method_replace"),
    # several guided concepts: each is appended unless the name so far CONTAINS it ("monet" is there from the concepts); the
    # lower-casing comes last
    (dict(concepts="monet, Dali", concept_type="other", guided_concepts="monet, Art"),
     "monet_dali-towards-art-preserve_false-sd_2_1-method_replace"),
    (dict(concepts="a, b", concept_type="object", guided_concepts="Sky, Sea", preserve_concepts="dog"),
     "a_b-towards-sky-sea-preserve_true-sd_2_1-method_replace"),
])
def test_names(kw, name):
    assert U.build_texts(artists=ARTISTS, **kw)[4] == name


# ---- the golden list
def test_golden_artist_list():
    with open(U.default_artists_file(), encoding="utf-8") as f:
        lines = f.read().split("\n")
    assert lines[-1] == "" and len(lines) == 1735
    names = lines[:-1]
    assert len(set(names)) == 1734 and all(n and n == n.strip() for n in names)
    assert names[:3] == ["A.J.Casson", "Aaron Douglas", "Aaron Horkey"] and U.read_artists() == names
    assert os.path.getsize(U.default_artists_file()) < 32 * 1024
    assert os.path.exists(os.path.join(os.path.dirname(U.default_artists_file()), "uce.report.txt"))


# ---- flags
def test_flags():
    s = _script()
    a = s.parse_args(["--concepts", "Picasso", "--guided_concept", "art", "--concept_type", "art"])        # run.sh's spelling
    assert a.guided_concepts == "art" and a.technique == "replace" and a.erase_scale == 1 and a.preserve_scale is None
    assert a.add_prompts is False and a.base == "2.1" and a.device == "0" and a.seed == 0 and a.output_dir == "."
    assert s.parse_args(["--concepts", "x", "--concept_type", "art", "--add_prompts", "False"]).add_prompts is True    # type=bool
    with pytest.raises(SystemExit):
        s.parse_args(["--concepts", "x"])                                # --concept_type is required
    assert "uce" in E.BASELINES
    E.check_baseline("uce", ckpt_name="models/erased-x.pt")


def test_kv_columns_tile_the_master_matrix():
    from types import SimpleNamespace
    from pdm.models.unet.params import build_entries
    from pdm.models.unet.spec import UNetConfig, apply_arch_vector, arch_vector_for_budget
    cfg = UNetConfig.tiny()
    entries = build_entries(cfg, apply_arch_vector(cfg, arch_vector_for_budget(cfg, 0.6, hw=16)[0]))
    unet = SimpleNamespace(store=SimpleNamespace(by_key={e.key: e for e in entries}))
    cols = U.kv_columns(unet)
    e = unet.store.by_key["attn2_kv_all.weight"]
    assert cols[0][1] == 0 and cols[-1][1] + cols[-1][2] == e.shape[0]
    assert all(a + r == b for (_n, a, r), (_m, b, _r) in zip(cols, cols[1:]))
    assert all(n.endswith(("attn2.to_k.weight", "attn2.to_v.weight")) for n, _a, _r in cols)
