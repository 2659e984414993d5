"""UCE debiasing, host side (no GPU): the text lists and checkpoint names of train_debias.py, the token windows of an old text
and its A attribute texts, the outer loop's bookkeeping (`schedule`) against the literal restatement of
tests/uce_debias_fixtures.py on hand-written ratio tables, the natural sort and column names of CLIP_classify.py, and the
professions fixture."""
import os

import pytest
import torch

import uce_debias_fixtures as fx
from pdm.utils import uce_debias as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def t(*v):
    return torch.tensor(v, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- texts and names
def test_build_texts_names_and_templates():
    old, new, retain, name = D.build_texts("Doctor, nurse", "male, female", professions=["doctor", "Nurse", "pilot", "CEO"])
    assert old == ["image of Doctor", "photo of Doctor", "portrait of Doctor", "picture of Doctor", "Doctor",
                   "image of nurse", "photo of nurse", "portrait of nurse", "picture of nurse", "nurse"]
    assert new[0] == ["image of male", "image of female"] and new[4] == ["male", "female"]
    assert new[7] == ["portrait of male", "portrait of female"]
    assert retain == ["pilot", "CEO"]                                  # `doctor` and `Nurse` equal an old text, case aside
    assert name == "doctor_nurse-attributes-male_female-sd_2_1"


def test_build_texts_single_attribute_is_duplicated_and_spaces_are_nines():
    old, new, _retain, name = D.build_texts("chef", "a Man", professions=["chef"])
    assert new == [[f"{p}a Man"] * 2 for p in ("image of ", "photo of ", "portrait of ", "picture of ", "")]
    assert name == "chef-attributes-a9man-sd_2_1"
    _old, new3, _r, name3 = D.build_texts("chef", "a, b c, d", professions=[])
    assert [len(n) for n in new3] == [3] * 5 and name3 == "chef-attributes-a_b9c_d-sd_2_1"


def test_build_texts_default0_and_retain_from_the_fixture():
    old, new, retain, name = D.build_texts("default0", "male, female")
    settings = D.load_settings()
    assert len(settings["default0"]) == 37 and len(old) == 37 * 5 and len(new) == len(old)
    assert old[:5] == ["image of attendant", "photo of attendant", "portrait of attendant", "picture of attendant", "attendant"]
    assert old[-1] == "chef" and "portrait of construction worker" in old and "CEO" in old
    assert name == "default0-attributes-male_female-sd_2_1"
    professions = D.read_professions()
    lower = {o.lower() for o in old}
    assert retain == [p for p in professions if p.lower() not in lower] and 0 < len(retain) < len(professions)
    assert (settings["max_bias_diff"], settings["weight_step"], settings["max_iterations"], settings["num_seeds"],
            settings["num_inference_steps"]) == (0.05, 0.1, 30, 5, 20)


@pytest.mark.parametrize("base", ["1.4", "2.0", "xl"])
def test_build_texts_other_bases_raise(base):
    with pytest.raises(NotImplementedError, match="only 2.1"):
        D.build_texts("chef", "male, female", professions=[], base=base)


def test_professions_fixture():
    path = os.path.join(ROOT, "tests", "golden", "uce", "professions.txt")
    assert D.default_professions_file() == path
    names = D.read_professions()
    assert len(names) >= 30 and len(set(names)) == len(names) and all(n == n.strip() and n for n in names)
    assert os.path.getsize(path) < 1 << 20


# ---------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("n_old,n_new", [(5, [4, 7, 5]), (9, [3, 4]), (3, [3, 3]), (4, [6]), (13, [13, 12, 11, 13])])
def test_group_slices(n_old, n_new):
    T = 13 if max(n_new + [n_old]) <= 13 else 77
    (a0, a1), news = D.group_slices(n_old, n_new, T)
    so, sn = fx.group_slices(n_old, n_new, T)
    assert (a0, a1) == (so.start, so.stop)
    assert news == [(s.start, s.stop) for s in sn]
    rows = a1 - a0
    assert rows == T - (max(n_new + [n_old]) - 2) and all(b1 - b0 == rows for b0, b1 in news)
    assert max([a1] + [b1 for _b0, b1 in news]) == T                  # the text that ends last reaches the end


def test_group_slices_is_pair_slices_for_one_new_text():
    from pdm.utils.uce import pair_slices
    for n_old, n_new in [(3, 9), (9, 3), (5, 5)]:
        a, (b,) = D.group_slices(n_old, [n_new], 77)
        assert (a, b) == pair_slices(n_old, n_new, 77)


# ---------------------------------------------------------------------------------------------- schedule
OLD = ["image of x", "photo of x", "x", "y"]


def _same(step, ratios, retain):
    done, weights, ret, change = fx.reference_schedule(ratios, retain, OLD)
    assert step.done == done
    assert [float(c) for c in step.max_change] == [float(c) for c in change]
    assert step.retain_texts == [str(r) for r in ret]
    if done:
        assert step.weights is None
    else:
        assert len(step.weights) == len(weights)
        for a, b in zip(step.weights, weights):
            assert a.dtype == torch.float32 and torch.equal(a, b)


def test_schedule_stops_below_the_gap():
    ratios = [t(0.52, 0.48), t(0.5, 0.5), t(0.46, 0.54), t(0.54, 0.46)]
    step = D.schedule(ratios, None, None, ["b", "a"], OLD)
    assert step.done and step.weights is None and step.retain_texts == ["b", "a"] and step.bypass == [True] * 4
    _same(step, ratios, ["b", "a"])


def test_schedule_weights_zeroed_and_retain_grows_sorted():
    ratios = [t(0.9, 0.1), t(0.52, 0.48), t(0.2, 0.8), t(0.5, 0.5)]
    retain = ["zebra", "apple", "apple"]
    step = D.schedule(ratios, None, None, retain, OLD)
    assert not step.done
    assert torch.equal(step.weights[0], 0.1 * (t(0.5, 0.5) - ratios[0])) and float(step.weights[0][0]) < 0 < float(step.weights[0][1])
    assert not step.weights[1].any() and not step.weights[3].any() and step.weights[2].any()
    # the attained texts join the list, which is then sorted and de-duplicated as np.unique leaves it
    assert step.retain_texts == ["apple", "photo of x", "y", "zebra"]
    assert step.bypass == [False, True, False, True]
    _same(step, ratios, retain)
    # nothing attained: the list is left exactly as it came, duplicates and order included
    step = D.schedule([t(0.9, 0.1), t(0.1, 0.9), t(0.3, 0.7), t(0.7, 0.3)], None, None, retain, OLD)
    assert step.retain_texts == retain and step.bypass == [False] * 4


def test_schedule_bypass_keeps_the_previous_ratio():
    prev = [t(0.9, 0.1), t(0.52, 0.48), t(0.2, 0.8), t(0.5, 0.5)]
    first = D.schedule(prev, None, None, [], OLD)
    measured = [t(0.8, 0.2), None, t(0.3, 0.7), t(0.0, 1.0)]          # the bypassed entries hold whatever
    step = D.schedule(measured, prev, first.max_change, first.retain_texts, OLD)
    assert torch.equal(step.ratios[1], prev[1]) and torch.equal(step.ratios[3], prev[3])
    assert torch.equal(step.ratios[0], measured[0]) and torch.equal(step.ratios[2], measured[2])
    _same(step, [measured[0], prev[1], measured[2], prev[3]], first.retain_texts)
    assert step.retain_texts == ["photo of x", "y"]                    # np.unique leaves the list as it was


def test_schedule_first_weight_zero_quirk():
    # three attributes, the first share exactly uniform: weights[c][0] == 0 although the concept is not debiased - the
    # reference adds the text to the retain list all the same, and keeps its other weights
    third = torch.ones(3) / 3
    ratios = [torch.stack([third[0], t(0.6)[0], 1 - third[0] - t(0.6)[0]]), t(0.9, 0.05, 0.05), t(0.8, 0.1, 0.1), t(0.1, 0.1, 0.8)]
    step = D.schedule(ratios, None, None, [], OLD)
    assert float(step.weights[0][0]) == 0 and float(step.weights[0][1]) != 0 and not step.bypass[0]
    assert step.retain_texts == ["image of x"]
    _same(step, ratios, [])


def test_schedule_ratio_exactly_at_the_boundary():
    # max |ratio - 1/A| == fp32(0.05) exactly: not "< 0.05", so the loop goes on and the text is measured again; not
    # "> 0.05", so its weights are zero and it joins the retain list.  With two attributes 1/2 -+ fp32(0.05) is no fp32 number;
    # with sixteen, 1/16 - fp32(0.05) is one, and the difference of two neighbours is exact.
    edge = torch.tensor(0.05, dtype=torch.float32)
    low = torch.tensor(0.0625) - edge
    at = torch.cat([low[None], torch.full((15,), float((1 - low) / 15))])
    assert float((at - torch.ones(16) / 16).abs().max()) == float(edge)
    step = D.schedule([at, at, at, at], None, None, [], OLD)
    assert not step.done and step.bypass == [False] * 4
    assert all(not w.any() for w in step.weights) and step.retain_texts == sorted(OLD)
    _same(step, [at] * 4, [])
    # one fp32 step of the difference (2^-28) further out the text is still biased, one step further in it is debiased
    out = at.clone()
    out[0] = low - 2.0 ** -28
    step = D.schedule([out, at, at, at], None, None, [], OLD)
    assert step.weights[0].any() and "image of x" not in step.retain_texts and not step.bypass[0]
    _same(step, [out, at, at, at], [])
    inn = at.clone()
    inn[0] = low + 2.0 ** -28
    step = D.schedule([inn, at, at, at], None, None, [], OLD)
    assert not step.weights[0].any() and step.bypass[0] and not step.done
    # 11 of 20 images with two attributes: fp32(0.55) - 0.5 lies above fp32(0.05)
    near = t(11, 9) / torch.tensor(20.0)
    assert D.schedule([near, near], None, None, [], OLD[:2]).weights[0].any()


# ---------------------------------------------------------------------------------------------- CLIP_classify.py
def test_sorted_nicely_and_columns():
    names = ["10_0.png", "2_1.png", "2_0.png", "1_0.png", "100_3.png"]
    assert D.sorted_nicely(names) == ["1_0.png", "2_0.png", "2_1.png", "10_0.png", "100_3.png"]
    assert [D.png_case_number(n) for n in ("12_3.png", "7.png")] == [12, 7]
    assert D.bias_columns(["a man", "a woman", "x"]) == ["a_man_bias", "a_woman_bias", "x_bias"]

