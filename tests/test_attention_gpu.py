"""Attention kernels (-m gpu): every dispatch form of csrc/attention.hip - 16 / 32 rows per wave in the forward, dQ and dK/dV
kernels, the query-split dK/dV, the causal forward - against an fp64 reference on planted-key inputs (tests/attention_fixtures.py).

Every call goes through _pdmk.attn_fwd / attn_bwd with the engine's stride patterns (fused q|k|v rows, ld = 3*H*64; a k|v
pair, ld = 2*H*64; dq / dk / dv written into column slices of the matching gradient buffers), every output buffer sits between
canary bands, and the form that ran is read back through _pdmk.attn_last_forms().  Bound: the error against fp64, in max-norm,
relative L2 and per row, is at most 8 x the error of an honest computation in the dtype's rounding policy (floor 8 ulp).
Each comparison prints an ATTN_PARITY line (measured / yardstick ratios; profiles/attn_parity.txt is a collected run)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_fixtures as af  # noqa: E402

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
VARS = ("PDMK_ATTN_NQ", "PDMK_ATTN_NQ_DQ", "PDMK_ATTN_NQ_DKV")
GUARD = 4096          # canary elements on either side of every output buffer
CANARY = 777.0


def _k():
    from pdm import _pdmk
    return _pdmk


@pytest.fixture
def force_forms():
    """Force the rows-per-wave form (1 = 16, 2 = 32) of the forward, dQ and dK/dV kernels; restored afterwards."""
    saved = {v: os.environ.get(v) for v in VARS}

    def setter(fwd, dq, dkv):
        for var, val in zip(VARS, (fwd, dq, dkv)):
            os.environ[var] = str(val)
    yield setter
    for var, val in saved.items():
        if val is None:
            os.environ.pop(var, None)
        else:
            os.environ[var] = val


# ------------------------------------------------------------------------------------------------ references, shared across forms
_CACHE = {}


def fixture_and_refs(dev, kind, B, H, Nq, Nk, dn, seed, causal=False):
    """(fixture, fp64 reference, yardstick) on the device, computed once per fixture; one slice of the reference is recomputed
    on the CPU (1e-12) so that it does not lean on the GPU's BLAS."""
    key = (kind, B, H, Nq, Nk, dn, seed, causal)
    if key not in _CACHE:
        while len(_CACHE) >= 3:
            _CACHE.pop(next(iter(_CACHE)))
        if kind == "rescale":
            fx = af.make_rescale(B, H, Nq, Nk, DT[dn], seed)
        else:
            fx = af.make_planted(B, H, Nq, Nk, kind, DT[dn], seed, causal)
        ref = af.reference(fx, dev)
        af.check_reference_slice(fx, ref, B - 1, H - 1)
        _CACHE[key] = (fx, ref, af.yardstick(fx, dev))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ launching
class Guarded:
    """A tensor of `shape` between two canary bands of one allocation."""

    def __init__(self, shape, dtype, dev):
        n = 1
        for d in shape:
            n *= d
        self.full = torch.full((n + 2 * GUARD,), CANARY, device=dev, dtype=dtype)
        self.t = self.full[GUARD:GUARD + n].view(*shape)

    def intact(self):
        band = torch.cat([self.full[:GUARD], self.full[-GUARD:]]).float()
        return bool((band == torch.tensor(CANARY, dtype=self.full.dtype).float().item()).all())


def _rows(x):       # [B, H, N, 64] -> [B, N, H*64]
    B, H, N, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, H * af.D)


def _slices(x, H):  # [B, N, H*64] -> [B*H, N, 64]
    B, N, _ = x.shape
    return x.reshape(B, N, H, af.D).permute(0, 2, 1, 3).reshape(B * H, N, af.D)


def run_kernels(fx, dev, backward=True, ws_elems=None):
    """Forward (+ backward) of `fx` through the C ABI in the engine's layouts.  Returns ({o, lse, dq, dk, dv as [B*H, N, 64] /
    [B*H, 1, Nq]}, forms after the forward, forms after the backward)."""
    k = _k()
    B, H, Nq, Nk, dt = fx.B, fx.H, fx.Nq, fx.Nk, fx.dtype
    d = H * af.D
    self_attn = Nq == Nk
    if self_attn:       # one fused projection output q|k|v per token; its gradient buffer has the same shape
        act = torch.cat([_rows(fx.q), _rows(fx.k), _rows(fx.v)], -1).to(dev).contiguous()
        q, kk, v = act[..., :d], act[..., d:2 * d], act[..., 2 * d:]
        grad = Guarded((B, Nq, 3 * d), dt, dev)
        dq, dk, dv = grad.t[..., :d], grad.t[..., d:2 * d], grad.t[..., 2 * d:]
        qs = ks = vs = dqs = dks = dvs = (Nq * 3 * d, 3 * d)
        guards = [grad]
    else:               # q from the latent tokens, k|v from one projection of the text tokens
        q = _rows(fx.q).to(dev).contiguous()
        kv = torch.cat([_rows(fx.k), _rows(fx.v)], -1).to(dev).contiguous()
        kk, v = kv[..., :d], kv[..., d:]
        gq, gkv = Guarded((B, Nq, d), dt, dev), Guarded((B, Nk, 2 * d), dt, dev)
        dq, dk, dv = gq.t, gkv.t[..., :d], gkv.t[..., d:]
        qs = dqs = (Nq * d, d)
        ks = vs = dks = dvs = (Nk * 2 * d, 2 * d)
        guards = [gq, gkv]
    o, lse = Guarded((B, Nq, d), dt, dev), Guarded((B, H, Nq), torch.float32, dev)
    guards += [o, lse]
    os_ = (Nq * d, d)
    if fx.causal:
        k.attn_fwd_causal(q, kk, v, o.t, lse.t, B, H, Nq, qs, ks, vs, os_, af.SCALE)
    else:
        k.attn_fwd(q, kk, v, o.t, lse.t, B, H, Nq, Nk, qs, ks, vs, os_, af.SCALE)
    f_fwd = k.attn_last_forms()
    got = {"o": _slices(o.t, H), "lse": lse.t.reshape(B * H, 1, Nq)}
    f_bwd = None
    if backward:
        do = _rows(fx.do).to(dev).contiguous()
        delta = Guarded((B, H, Nq), torch.float32, dev)
        guards.append(delta)
        k.attn_bwd(q, kk, v, o.t, do, lse.t, delta.t, dq, dk, dv, B, H, Nq, Nk, qs, ks, vs, os_, dqs, dks, dvs, af.SCALE,
                   ws_elems=ws_elems)
        f_bwd = k.attn_last_forms()
        got.update(dq=_slices(dq, H), dk=_slices(dk, H), dv=_slices(dv, H))
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), "a canary band around an output buffer was overwritten"
    return got, f_fwd, f_bwd


def check(tag, fx, ref, yard, got, rows=None, tensors=None):
    fails = []
    for t in tensors or [t for t in af.TENSORS if t in got]:
        ok, line, _ = af.compare(t, got[t], ref[t], yard[t], fx.dtype, rows)
        print("ATTN_PARITY", tag, line)
        if not ok:
            fails.append(f"{tag} {line}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ automatic dispatch
@pytest.mark.parametrize("regime", ["peaked", "mid"])
@pytest.mark.parametrize("B,H,Nq,Nk,dn,fwd,dq,dkv,nsplit", af.PRODUCTION_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[4]}" for c in af.PRODUCTION_CASES])
def test_production_shapes_take_the_expected_forms(dev, regime, B, H, Nq, Nk, dn, fwd, dq, dkv, nsplit):
    """The shapes the benchmark and the trainer run, with the library's own dispatch (nothing forced): the wide forward / dQ /
    dK/dV at (8, 5, 4096^2), (8, 10, 1024^2) and exactly at the thresholds (16, 20, 256^2); narrow just under them; fp32 wide in
    the forward only; cross-attention with and without the query split."""
    fx, ref, yard = fixture_and_refs(dev, regime, B, H, Nq, Nk, dn, af.seed_for(Nq, Nk, regime))
    got, f_fwd, f_bwd = run_kernels(fx, dev)
    assert f_fwd[0] == fwd, f"forward form {f_fwd[0]}, expected {fwd}"
    assert f_bwd[1:] == (dq, dkv, nsplit), f"(dQ, dK/dV, nsplit) = {f_bwd[1:]}, expected {(dq, dkv, nsplit)}"
    check(f"auto {B}x{H}x{Nq}x{Nk} {dn} {regime} forms={f_fwd[0]}{f_bwd[1]}{f_bwd[2]} nsplit={f_bwd[3]}", fx, ref, yard, got)


# ------------------------------------------------------------------------------------------------ forced forms, ragged shapes
FORMS = [(f, q, kv) for f in (1, 2) for q in (1, 2) for kv in (1, 2) if (f, q, kv) != (1, 1, 1)]


@pytest.mark.parametrize("regime", ["peaked", "mid"])
@pytest.mark.parametrize("forms", FORMS, ids=["fwd%d-dq%d-dkv%d" % f for f in FORMS])
@pytest.mark.parametrize("N", af.RAGGED_N)
def test_forced_forms_on_ragged_shapes(dev, force_forms, N, forms, regime):
    """N % 128 in 1..64 leaves the second 16-row tile of every wave of a wide kernel empty, 65..127 leaves it ragged; the same for
    the keys of the wide dK/dV kernel.  Mixed dQ / dK/dV forms: dK/dV reads the delta that the dQ kernel publishes."""
    fx, ref, yard = fixture_and_refs(dev, regime, 2, 3, N, N, "bf16", af.seed_for(N, N, regime))
    force_forms(*forms)
    got, f_fwd, f_bwd = run_kernels(fx, dev)
    assert (f_fwd[0], f_bwd[1], f_bwd[2]) == forms and f_bwd[3] == 1, (f_fwd, f_bwd)
    check(f"forced 2x3x{N}x{N} bf16 {regime} forms={forms[0]}{forms[1]}{forms[2]}", fx, ref, yard, got)


@pytest.mark.parametrize("regime", ["peaked", "mid"])
@pytest.mark.parametrize("N", af.RAGGED_N)
def test_forced_wide_forward_fp32(dev, force_forms, N, regime):
    """fp32 has a wide form in the forward only; its backward stays narrow whatever is forced (not forced here)."""
    fx, ref, yard = fixture_and_refs(dev, regime, 2, 3, N, N, "f32", af.seed_for(N, N, regime))
    force_forms(2, 1, 1)
    got, f_fwd, f_bwd = run_kernels(fx, dev)
    assert f_fwd[0] == 2 and f_bwd[1:] == (1, 1, 1), (f_fwd, f_bwd)
    check(f"forced 2x3x{N}x{N} f32 {regime} forms=211", fx, ref, yard, got)


@pytest.mark.parametrize("regime", ["peaked", "mid"])
@pytest.mark.parametrize("Nq,Nk", af.RAGGED_CROSS)
def test_forced_wide_dq_on_cross_shapes(dev, force_forms, Nq, Nk, regime):
    fx, ref, yard = fixture_and_refs(dev, regime, 2, 3, Nq, Nk, "bf16", af.seed_for(Nq, Nk, regime))
    force_forms(1, 2, 1)
    got, f_fwd, f_bwd = run_kernels(fx, dev)
    assert f_fwd[0] == 1 and f_bwd[1:] == (2, 1, 1), (f_fwd, f_bwd)
    check(f"forced 2x3x{Nq}x{Nk} bf16 {regime} forms=121", fx, ref, yard, got)


# ------------------------------------------------------------------------------------------------ online-softmax rescale
@pytest.mark.parametrize("dn", ["bf16", "f32"])
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("Nk", af.RESCALE_NK)
def test_lazy_rescale_moves_and_stays(dev, force_forms, Nk, form, dn):
    """Rows whose running reference moves over NON-ZERO accumulators (the alpha < 1 multiply of ot / ol), and rows where a
    block exceeds the reference by 4..8 and it must stay (probabilities up to 2^8): o and lse are bounded on each set of rows
    separately as well as overall."""
    Nq = min(Nk, 1024)
    fx, ref, yard = fixture_and_refs(dev, "rescale", 2, 3, Nq, Nk, dn, af.RESCALE_SEED)
    moved, under = af.rescale_rows(fx, af.KVB[DT[dn]], dev)
    assert moved.float().mean() >= 0.10 and under.float().mean() >= 0.05
    wide_bwd = form if dn == "bf16" else 1
    force_forms(form, wide_bwd, wide_bwd)
    got, f_fwd, f_bwd = run_kernels(fx, dev)
    assert f_fwd[0] == form and f_bwd[1:3] == (wide_bwd, wide_bwd), (f_fwd, f_bwd)
    tag = f"rescale 2x3x{Nq}x{Nk} {dn} forms={form}{wide_bwd}{wide_bwd}"
    check(tag, fx, ref, yard, got)
    check(tag + " moved-rows", fx, ref, yard, got, rows=moved, tensors=("o", "lse"))
    check(tag + " under-8-rows", fx, ref, yard, got, rows=under, tensors=("o", "lse"))


# ------------------------------------------------------------------------------------------------ workspace clamp
@pytest.mark.parametrize("share,nsplit", [("all", 16), ("half", 8), ("none", 1)])
def test_dkv_split_is_clamped_to_the_workspace(dev, share, nsplit):
    """(1, 2, 4096, 77) asks for 16 query splits; with half of pdmk_attn_bwd_workspace_bytes the split is 8, with no workspace
    there is none - same bound."""
    k = _k()
    B, H, Nq, Nk = af.CLAMP_SHAPE
    fx, ref, yard = fixture_and_refs(dev, "mid", B, H, Nq, Nk, "bf16", af.CLAMP_SEED)
    full = int(k._lib.pdmk_attn_bwd_workspace_bytes(B, H, Nq, Nk)) // 4
    assert full == 16 * 2 * B * H * Nk * 64
    got, _, f_bwd = run_kernels(fx, dev, ws_elems={"all": None, "half": full // 2, "none": 0}[share])
    assert f_bwd[3] == nsplit and f_bwd[2] == 1, f_bwd
    check(f"clamp {B}x{H}x{Nq}x{Nk} bf16 mid ws={share} nsplit={f_bwd[3]}", fx, ref, yard, got)


# ------------------------------------------------------------------------------------------------ causal forward
@pytest.mark.parametrize("dn", ["bf16", "f32"])
@pytest.mark.parametrize("N", af.CAUSAL_N)
def test_causal_forward(dev, N, dn):
    """attn_fwd_causal with planted keys pi(i) <= i."""
    fx, ref, yard = fixture_and_refs(dev, "peaked", 2, 3, N, N, dn, af.causal_seed(N), causal=True)
    got, f_fwd, _ = run_kernels(fx, dev, backward=False)
    assert f_fwd[0] == 1
    check(f"causal 2x3x{N}x{N} {dn} peaked forms=1", fx, ref, yard, got)
