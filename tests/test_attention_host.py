"""Conditions on the attention fixtures themselves (no GPU): for every fixture and regime tests/test_attention_gpu.py uses, at
a reduced B * H (the leading slices of the same draw), the fp64 reference alone must show that the fixture can see what it
is there to see -

* the median row-maximum probability sits in the regime's band;
* the rescale variant has >= 10 % of rows whose running softmax reference moves after the first key block and >= 5 % where a
  later block exceeds it by 4..8 without moving it, for the key-block size of either dtype;
* what a kernel that drops the last key, drops the last query or exchanges two V rows of a tile WOULD compute differs from
  the reference by at least 3 x the bound the GPU test applies to the tensor that mistake should show in (o for a dropped
  key or exchanged V rows when peaked, dv for a dropped query, dq or dk for a dropped key when mid).  The GPU test asserts
  three statistics per tensor, so a mistake is caught when any one of them is exceeded: the largest ratio counts.
  (For a dropped key the surviving keys' dk rows move little by construction - the lost probability mass spreads over all
  the other keys of that one query - so it is that query's dq row which has to carry the signal; both are accepted.)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_fixtures as af  # noqa: E402

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
MARGIN = 3.0


def margin(fx, ref, yard, mutated, keep, tensors):
    """Largest (mutation effect / GPU-test bound) over the given tensors and the three statistics."""
    best = 0.0
    for t in tensors:
        eff = af.mutation_effect(t, ref, mutated, keep[t])
        bd, _ = af.bounds(t, ref[t], yard[t], fx.dtype)
        best = max(best, max(eff[s] / bd[s] for s in af.STATS))
    return best


def sensitivities(fx):
    ref, yard = af.reference(fx), af.yardstick(fx)
    out = {}
    m, keep = af.mutate_delete_last_key(fx)
    out["key->o"] = margin(fx, ref, yard, m, keep, ("o",))
    out["key->dq|dk"] = margin(fx, ref, yard, m, keep, ("dq", "dk"))
    if not fx.causal:
        m, keep = af.mutate_delete_last_query(fx)
        out["query->dv"] = margin(fx, ref, yard, m, keep, ("dv",))
    m, keep = af.mutate_swap_v_rows(fx, *af.swap_pair(fx))
    out["vswap->o"] = margin(fx, ref, yard, m, keep, ("o",))
    return out


REQUIRED = {"peaked": ("key->o", "vswap->o", "query->dv"), "mid": ("query->dv", "key->dq|dk")}
SHAPES = sorted({(c[2], c[3], c[4]) for c in af.PRODUCTION_CASES} | {(n, n, d) for n in af.RAGGED_N for d in ("bf16", "f32")} |
                {(q, k, "bf16") for q, k in af.RAGGED_CROSS})


@pytest.mark.parametrize("regime", ["peaked", "mid"])
@pytest.mark.parametrize("Nq,Nk,dn", SHAPES, ids=[f"{q}x{k}-{d}" for q, k, d in SHAPES])
def test_planted_fixture_is_in_band_and_sensitive(Nq, Nk, dn, regime):
    fx = af.make_planted(1, 1, Nq, Nk, regime, DT[dn], af.seed_for(Nq, Nk, regime))
    assert not bool((fx.pi == torch.arange(Nq)).all())
    assert set(af.required_keys(Nk)) <= set(fx.pi.tolist()), "pi misses a block edge"
    pm = af.pmax_median(fx)
    lo, hi = af.PMAX_BAND[regime]
    sens = sensitivities(fx)
    print(f"{regime} {Nq}x{Nk} {dn}: a = {fx.gain:.3f}, median pmax {pm:.3f}, margins {sens}")
    assert lo <= pm <= hi, f"median row-max probability {pm:.3f} outside {lo}-{hi}"
    for what in REQUIRED[regime]:
        assert sens[what] >= MARGIN, f"{what}: only {sens[what]:.2f} x the GPU test's bound"


@pytest.mark.parametrize("dn", ["bf16", "f32"])
@pytest.mark.parametrize("Nk", af.RESCALE_NK)
def test_rescale_fixture_moves_and_stays(Nk, dn):
    fx = af.make_rescale(1, 2, min(Nk, 1024), Nk, DT[dn], af.RESCALE_SEED)
    for kvb in sorted(set(af.KVB.values())):
        moved, under = af.rescale_rows(fx, kvb)
        mv, un = moved.float().mean().item(), under.float().mean().item()
        print(f"rescale Nk = {Nk} {dn}, key blocks of {kvb}: moved {mv:.3f}, 4..8 under {un:.3f}")
        assert mv >= 0.10 and un >= 0.05
    # the late rows' planted key is in the last key block of either size
    late = torch.arange(fx.Nq) % 20 < 7
    assert bool((fx.pi[late] >= (Nk - 1) // 32 * 32).all())


@pytest.mark.parametrize("dn", ["bf16", "f32"])
@pytest.mark.parametrize("N", af.CAUSAL_N)
def test_causal_fixture_is_in_band_and_sensitive(N, dn):
    fx = af.make_planted(1, 2, N, N, "peaked", DT[dn], af.causal_seed(N), causal=True)
    assert bool((fx.pi <= torch.arange(N)).all()) and not bool((fx.pi == torch.arange(N)).all())
    assert int(fx.pi[-1]) == N - 1
    pm = af.pmax_median(fx)
    sens = sensitivities(fx)
    print(f"causal {N} {dn}: median pmax {pm:.3f}, margins {sens}")
    lo, hi = af.PMAX_BAND["peaked"]
    assert lo <= pm <= hi
    assert sens["key->o"] >= MARGIN and sens["vswap->o"] >= MARGIN


def test_clamp_fixture_is_the_cross_attention_one():
    B, H, Nq, Nk = af.CLAMP_SHAPE
    assert (Nq, Nk) == (4096, 77) and af.CLAMP_SEED == af.seed_for(4096, 77, "mid")   # conditions asserted above


def test_reduced_fixture_is_the_leading_slice_of_the_full_one():
    small, full = af.make_planted(1, 1, 129, 77, "mid", torch.bfloat16, 5), af.make_planted(2, 3, 129, 77, "mid", torch.bfloat16, 5)
    for a, b in zip(small.slice(0, 0), full.slice(0, 0)):
        assert torch.equal(a, b)
    assert torch.equal(small.pi, full.pi)


def test_policy_twin_and_reference_agree_to_bf16_rounding():
    """The yardstick must itself be an accurate computation: within 2e-2 of fp64 in max-norm on a mid fixture."""
    fx = af.make_planted(1, 2, 200, 77, "mid", torch.bfloat16, 3)
    ref, yard = af.reference(fx), af.yardstick(fx)
    for t in af.TENSORS:
        assert af.error_stats(yard[t], ref[t])["max"] <= 2e-2, t
