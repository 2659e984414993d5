"""VAE / CLIP encoder kernels (csrc/encoders.hip: pdmk_softmax_rows, pdmk_latent_sample, pdmk_embed_tokens; csrc/clip.hip:
pdmk_patch_im2col, pdmk_vit_tokens, pdmk_quick_gelu_fwd, pdmk_gather_rows, pdmk_clip_score_head): every form of the row softmax
and its boundaries, every capped grid-stride loop past its first pass, vector lengths past one block, strided operands, both
storage types and every pointer mode, against float64 on the CPU or plain torch indexing.

Launch rules.  The five grid-stride kernels run `for (i = blockIdx.x * 256 + tid; i < items; i += gridDim.x * 256)` behind
grid = min(cap, ceil(items / 256)) with cap = 4096 (latent_sample) or 8192 (embed_tokens, im2col, vit_tokens, quick_gelu);
_items restates the item count of each entry point.  ENC_LARGE holds, per entry point and storage type, the smallest shapes
that reach the capped grid and take a second pass that ends neither on a block boundary nor on a pass boundary;
test_large_cases_reach_the_second_pass checks the table on a machine without a GPU.  pdmk_softmax_rows keeps a row in
registers, PER = 1, 2, 4 or 16 float4 per thread for cols <= 1024, 2048, 4096, 16384 (_softmax_per); SOFTMAX_COLS holds both
sides of every boundary.  pdmk_gather_rows and pdmk_clip_score_head walk a row with `c += 256`: D = 257 ... 1000 take 2 to 4
trips.  test_restated_constants_are_the_sources checks the restated caps and thresholds against the two source files.

References.  Kernels that only move or add values get integer inputs whose results are exact in the storage type and are
compared with torch.equal (embed_tokens, im2col, vit_tokens, gather_rows, the large latent_sample with logvar = 0 and a
power-of-two scale, and the 0 / +-1 case of the score head: 256 non-zeros per row, so every norm is 16, every quotient
+-1/16 and every dot product a multiple of 1/256).  Softmax, the small latent_sample shapes, QuickGELU and the score head on
random rows are compared with float64 on the CPU at the bounds the older tests of these entry points hold against device
torch (test_vae_gpu.py, test_clip_model_gpu.py, TOL of test_erasure_kernels_gpu.py); each prints an ENC_PARITY line before it
asserts (profiles/skinny_encoder_parity.txt is a collected run), and each first asserts its fixture: the same formula in fp32
on the CPU is within half the bound.  A bound is a fraction of a block's largest reference value, so each kind of value is a
block with a scale of its own: softmax rows with a +80 logit (slot and last-column reads, maximum subtraction) and plain
randn * 6 rows (the exponential and the normalisation); the latent pixels at the upper logvar clamp, below it, and at the
lower clamp; QuickGELU with and without the +-100 points.  The large QuickGELU launch must also equal, bit for bit, the same entry point run over
slices that fit in one pass.

Canaries.  Padding the kernels may read holds 1e6 (1e30 behind the softmax scores, where a read past `cols` would win the
maximum); every output is surrounded by sentinels - padding columns, rows after the last, elements after n, outputs that were
not requested - which must come back bit-identical.  One zero-fill is part of the interface and asserted as zeros: the columns
[K, ldo) of pdmk_patch_im2col."""
import functools
import os
import re

import pytest
import torch

from test_erasure_kernels_gpu import TOL as COS_TOL
from test_kernels_gpu import DT

NT = 256
V = {"bf16": 8, "f32": 4}
BOTH = ("bf16", "f32")
SENT = -123.0                     # 7 significant bits: exact in bf16
POISON = 1e6
GUARD, ROWS_AFTER = 64, 3
CAPS = {"latent_sample": 4096, "embed_tokens": 8192, "im2col": 8192, "vit_tokens": 8192, "quick_gelu": 8192}
SOFTMAX_MAX = 16384
SOFTMAX_COLS = (4, 64, 1000, 1024, 1028, 2048, 2052, 4096, 4100, 9000, 16384)
SOFTMAX_TOL = {"f32": 1e-5, "bf16": 1e-2}          # of the largest probability (test_softmax_rows); |sum - 1| < 1e-5 in fp32
GELU_TOL = {"f32": 2e-6, "bf16": 1e-2}             # of the output scale (test_quick_gelu)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unlearn-ft_amd", "csrc")


def _items(entry, dn, p):
    """items the grid-stride loop of one launch walks"""
    if entry == "latent_sample":
        return p["B"] * p["C"] * p["HW"]
    if entry == "embed_tokens":
        return p["B"] * p["T"] * (p["D"] // V[dn])
    if entry == "im2col":
        return p["B"] * (p["S"] // p["p"]) ** 2 * p["ldo"]
    if entry == "vit_tokens":
        return p["B"] * (p["G2"] + 1) * p["E"]
    if entry == "quick_gelu":
        return p["n"]
    raise KeyError(entry)


def _grid(entry, items):
    return min(CAPS[entry], -(-items // NT))


def _softmax_per(cols):
    """PER of softmax_launch (None: refused)"""
    for per in (1, 2, 4, 16):
        if cols <= NT * 4 * per:
            return per
    return None


ENC_LARGE = (
    [("latent_sample", dn, dict(B=2, C=4, HW=131109, ld=12)) for dn in BOTH]
    + [("embed_tokens", "bf16", dict(B=6809, T=77, D=32, vocab=50)), ("embed_tokens", "f32", dict(B=3405, T=77, D=32, vocab=50))]
    + [("im2col", dn, dict(B=14, S=224, p=32, ldo=3 * 32 * 32 + 8)) for dn in BOTH]
    + [("vit_tokens", dn, dict(B=437, G2=49, E=96)) for dn in BOTH]
    + [("quick_gelu", dn, dict(n=2097152 + 300)) for dn in BOTH]
)


def _large(entry, dn):
    out = [p for e, d, p in ENC_LARGE if e == entry and d == dn]
    assert len(out) == 1, (entry, dn)
    return out[0]


def _id(a):
    return "-".join(f"{x}{y}" for x, y in a.items()) if isinstance(a, dict) else str(a)


# ------------------------------------------------------------------------------------------------ host-only checks
def test_large_cases_reach_the_second_pass():
    """Host only: every shape of ENC_LARGE reaches the capped grid and a second pass that ends neither on a block boundary nor
    on a pass boundary; no smaller batch of the same shape does."""
    for entry, dn, p in ENC_LARGE:
        items = _items(entry, dn, p)
        what = (entry, dn, _id(p))
        cap = CAPS[entry]
        assert _grid(entry, items) == cap and items > cap * NT, what
        last = items % (cap * NT)
        assert last != 0 and last % NT != 0, what
        assert items < 2 * cap * NT, what                           # exactly two passes
        if "B" in p:                                                # the smallest batch that does it
            assert _items(entry, dn, dict(p, B=p["B"] - 1)) <= cap * NT, what
    assert {(e, d) for e, d, _ in ENC_LARGE} == {(e, d) for e in CAPS for d in BOTH}
    p = _large("im2col", "f32")
    assert p["ldo"] > 3 * p["p"] ** 2 and p["S"] % p["p"] == 0
    p = _large("latent_sample", "bf16")
    assert p["HW"] % 2 == 1 and p["ld"] > 2 * p["C"]
    # exact arithmetic: |mean|, |eps| <= 8 and scale = 1/4: multiples of 1/4 up to 4; token + position rows: |sum| <= 16
    assert (8 + 8) / 0.25 < 256 and 8 + 8 < 256


def test_softmax_columns_reach_every_form_and_boundary():
    """Host only: SOFTMAX_COLS has both sides of every form boundary, the one-thread row and the widest row; 16388 is refused"""
    per = {c: _softmax_per(c) for c in SOFTMAX_COLS}
    assert all(c % 4 == 0 for c in SOFTMAX_COLS) and set(per.values()) == {1, 2, 4, 16}
    for lo, hi in ((1, 2), (2, 4), (4, 16)):
        edge = NT * 4 * lo
        assert per[edge] == lo and per[edge + 4] == hi, edge
    assert per[4] == 1 and per[SOFTMAX_MAX] == 16 and _softmax_per(SOFTMAX_MAX + 4) is None
    assert per[1028] == 2 and per[2048] == 2                        # PER = 2: one thread in its second slot, and every thread
    assert 1000 % (4 * 64) and 9000 % (4 * NT)                      # a partly filled wave; a partly filled slot of PER = 16
    for cols in SOFTMAX_COLS:                                       # the dominant logits of a 5-row block: distinct slots, and the last column
        at = _dominant_columns(cols, 5)
        assert at[0] == cols - 1 and all(0 <= c < cols for c in at)
        slots = {c // (4 * NT) for c in at}
        assert len(slots) == min(5, -(-cols // (4 * NT))), (cols, at)


def test_restated_constants_are_the_sources():
    """Host only: the caps and thresholds the tables are built from are the ones in encoders.hip and clip.hip (a changed cap or
    form threshold there must be followed here, or the tables no longer reach what they list)."""
    enc = open(os.path.join(CSRC, "encoders.hip")).read()
    clip = open(os.path.join(CSRC, "clip.hip")).read()
    assert "constexpr int NT = 256;" in enc and "constexpr int NT = 256;" in clip
    assert [int(x) for x in re.findall(r"if \(cols <= NT \* (\d+)\)", enc)] == [4, 8, 16, 64]
    assert [int(x) for x in re.findall(r"softmax_rows_kernel<T, (\d+)>\)", enc)] == [1, 2, 4, 16]
    assert re.search(r"\(n \+ NT - 1\) / NT < 4096 \? \(n \+ NT - 1\) / NT : 4096", enc)                 # latent_sample
    assert re.search(r"\(items \+ NT - 1\) / NT < 8192 \? \(items \+ NT - 1\) / NT : 8192", enc)         # embed_tokens
    assert re.search(r"const long g = \(n \+ NT - 1\) / NT;\s*return \(unsigned\)\(g < 8192 \? g : 8192\);", clip)
    assert clip.count("dim3(grid_for(") == 3                                                            # im2col, vit_tokens, quick_gelu
    assert len(re.findall(r"i \+= \(long\)gridDim\.x \* NT", enc)) == 2 and len(re.findall(r"i \+= \(long\)gridDim\.x \* NT", clip)) == 3


def _dominant_columns(cols, rows):
    """Column of the +80 logit of each row: the last column in row 0, then one column in each of up to four other PER slots"""
    nslots = -(-cols // (4 * NT))
    others = max(1, nslots - 1)               # the slots before the last one (the only slot where there is one)
    at = [cols - 1]
    for r in range(1, rows):
        slot = ((r - 1) * others) // 4 if others >= 4 else (r - 1) % others
        lo = slot * 4 * NT
        at.append(lo + (37 * r + 1) % (min(cols, lo + 4 * NT) - lo))
    return at


SOFTMAX_KINDS = ("peaked", "plain")


@functools.lru_cache(maxsize=None)
def _softmax_case(cols, rows, kind):
    """(scores [rows, cols] fp32 on the CPU, fp64 softmax).  "peaked": a +80 logit per row (the row maximum must be subtracted,
    and the slot and the last column it sits in must be read): every other probability is below 1e-20, so this block says
    nothing about the exponential or the normalisation.  "plain": randn * 6 alone, a block of its own with a scale of its
    own, in which several probabilities per row are within 1e-3 of the largest."""
    g = torch.Generator().manual_seed(cols * 8 + rows + (100003 if kind == "plain" else 0))
    s = torch.randn(rows, cols, generator=g) * 6.0
    if kind == "peaked":
        for r, c in enumerate(_dominant_columns(cols, rows)):
            s[r, c] = 80.0
    return s, torch.softmax(s.double(), dim=-1)


def _softmax_err(p, ref):
    return float((p.double() - ref).abs().max()) / float(ref.max())


@pytest.mark.parametrize("kind", SOFTMAX_KINDS)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_fixture_fp32_is_within_half_the_bounds(cols, rows, kind):
    """Host only: fp32 softmax on the CPU, stored in either type, is within half of each bound the GPU test holds; the plain
    rows are sensitive to the arithmetic: a wrong base or scale of the exponential, or a one-hot at the maximum, is far outside"""
    s, ref = _softmax_case(cols, rows, kind)
    if kind == "plain" and cols >= 64:
        sd = s.double() - s.double().max(-1, keepdim=True).values
        for wrong in (torch.softmax(sd * 0.6931471805599453, -1), torch.softmax(sd * 0.9, -1), (sd == 0).double()):
            assert _softmax_err(wrong, ref) > SOFTMAX_TOL["bf16"], (cols, rows)
        assert int((ref >= 1e-3 * ref.max()).sum()) >= 4 * rows
    p32 = torch.softmax(s, dim=-1)
    assert _softmax_err(p32, ref) <= SOFTMAX_TOL["f32"] / 2
    assert _softmax_err(p32.bfloat16(), ref) <= SOFTMAX_TOL["bf16"] / 2
    assert float((p32.double().sum(-1) - 1).abs().max()) < 1e-5 / 2


def _gelu_points():
    return torch.tensor([0.0, 0.5, -0.5, 20.0, -20.0, 100.0, -100.0])


@functools.lru_cache(maxsize=None)
def _gelu_case(n, dn):
    """(x rounded to the storage type, fp64 x * sigmoid(1.702 x) of it); the fixed points come first where n allows"""
    g = torch.Generator().manual_seed(n)
    x = torch.cat([_gelu_points(), torch.randn(n, generator=g) * 4])[:n].to(DT[dn])
    xd = x.double()
    return x, xd * torch.sigmoid(1.702 * xd)


def _gelu_errs(y, ref):
    """max error over the output scale: of the whole tensor, and of the random part alone (the +-100 points set the first scale)"""
    e = (y.double() - ref).abs()
    npts = len(_gelu_points())
    out = [float(e.max()) / (float(ref.abs().max()) + 1e-6)]
    if ref.numel() > npts:
        out.append(float(e[npts:].max()) / (float(ref[npts:].abs().max()) + 1e-6))
    return out


GELU_N = (1, 7, 255, 256, 257)


@pytest.mark.parametrize("dn", BOTH)
@pytest.mark.parametrize("n", GELU_N)
def test_quick_gelu_fixture_fp32_is_within_half_the_bounds(n, dn):
    """Host only"""
    x, ref = _gelu_case(n, dn)
    y = (x.float() * torch.sigmoid(1.702 * x.float())).to(DT[dn])
    assert max(_gelu_errs(y, ref)) <= GELU_TOL[dn] / 2


# ------------------------------------------------------------------------------------------------ helpers of the GPU tests
def _ints(shape, dev, dt, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, tuple(shape), device=dev).to(dt)


def _guarded(n, dev, dt):
    """exactly n elements with GUARD sentinel elements on either side; the view stays 16-byte aligned"""
    buf = torch.full((n + 2 * GUARD,), SENT, device=dev, dtype=dt)
    view = buf[GUARD:GUARD + n]
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_intact(buf, n, what):
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all()), what + ": written outside its n elements"


def _out_rows(rows, cols, ld, dev, dt):
    """a [rows, cols] view with row stride ld, sentinels in the padding columns and in ROWS_AFTER rows after it"""
    buf = torch.full((rows + ROWS_AFTER, ld), SENT, device=dev, dtype=dt)
    return buf, buf[:rows, :cols]


def _pads_intact(buf, rows, cols, what):
    assert bool((buf[:rows, cols:] == SENT).all()), what + ": padding columns written"
    assert bool((buf[rows:] == SENT).all()), what + ": rows after the last written"


def _in_rows(vals, ld, fill=POISON, rows_after=ROWS_AFTER):
    """vals [rows, cols] as a view of a [rows + rows_after, ld] buffer of the same type and device; the rest holds `fill`"""
    rows, cols = vals.shape
    buf = torch.full((rows + rows_after, ld), fill, device=vals.device, dtype=vals.dtype)
    buf[:rows, :cols] = vals
    return buf, buf[:rows, :cols]


def _parity(entry, dn, shape, err, tol):
    print(f"ENC_PARITY {entry} {dn} {shape} err={err:.3e} tol={tol:.1e}")
    assert err == err and err <= tol, f"{entry} {dn} {shape}: error {err:.3e} over {tol:.1e}"


# ------------------------------------------------------------------------------------------------ softmax
@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("kind", SOFTMAX_KINDS)
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_rows_forms(dev, cols, kind, rows, dn):
    from pdm import _pdmk as k
    s, ref = _softmax_case(cols, rows, kind)
    p32 = torch.softmax(s, dim=-1)                                  # the fixture: fp32 on the CPU is within half of each bound
    assert _softmax_err(p32.to(DT[dn]), ref) <= SOFTMAX_TOL[dn] / 2 and float((p32.double().sum(-1) - 1).abs().max()) < 1e-5 / 2
    lds, ldp = cols + 4, cols + 3
    assert ldp % 2 == 1
    sbuf, _ = _in_rows(s.to(dev), lds, fill=1e30)
    pbuf, p = _out_rows(rows, cols, ldp, dev, DT[dn])
    k.softmax_rows(sbuf, pbuf, rows, cols, lds, ldp)
    what = f"cols={cols} rows={rows} PER={_softmax_per(cols)}"
    got = p.cpu()
    _parity("softmax_rows_" + kind, dn, what, _softmax_err(got, ref), SOFTMAX_TOL[dn])
    if dn == "f32":
        _parity("softmax_rows_" + kind + "_sum", dn, what, float((got.double().sum(-1) - 1).abs().max()), 1e-5)
    _pads_intact(pbuf, rows, cols, "softmax_rows " + what)


@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
@pytest.mark.parametrize("cols", [c for c in SOFTMAX_COLS if c & (c - 1) == 0])
def test_softmax_uniform_row_is_exact(dev, cols, dn):
    """An all-equal row at a power-of-two width: exp2(0) = 1, the sum is cols, every probability exactly 1 / cols"""
    from pdm import _pdmk as k
    s = torch.full((2, cols + 4), 1e30, device=dev)
    s[0, :cols] = -3.75
    s[1, :cols] = 11.0
    pbuf, p = _out_rows(2, cols, cols + 3, dev, DT[dn])
    k.softmax_rows(s, pbuf, 2, cols, cols + 4, cols + 3)
    assert torch.equal(p, torch.full_like(p, 1.0 / cols)), f"cols={cols}"
    _pads_intact(pbuf, 2, cols, f"uniform cols={cols}")


# ------------------------------------------------------------------------------------------------ latent sample
def _latent_ref(mom, eps, B, Cc, HW, scale):
    """fp64 (mean + exp(logvar / 2) eps) * scale, logvar clamped to [-30, 20], NHWC moments -> NCHW latents"""
    m = mom.double().view(B, HW, -1)
    mean, logvar = m[..., :Cc].permute(0, 2, 1), m[..., Cc:2 * Cc].permute(0, 2, 1).clamp(-30.0, 20.0)
    s = float(torch.tensor(scale, dtype=torch.float32))               # the entry point takes a float
    return (mean + torch.exp(0.5 * logvar) * eps.double().view(B, Cc, HW)) * s


@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
@pytest.mark.parametrize("Cc,pad", [(3, 0), (3, 5), (4, 0), (4, 24)])
def test_latent_sample_small(dev, dn, Cc, pad):
    """C = 3 and 4, odd HW, ld = 2 C and ld > 2 C (1e6 behind the moments), both clamp ends, against fp64 at 1e-5 of the scale of
    the whole output, of the pixels below the upper clamp, and of the pixels at the lower clamp"""
    from pdm import _pdmk as k
    B, HW, ld = 3, 35, 2 * Cc + pad
    g = torch.Generator().manual_seed(Cc * 100 + pad)
    vals = torch.randn(B * HW, 2 * Cc, generator=g) * 3.0
    vals[0, Cc:] = torch.tensor([-100.0, -30.0, 20.0, 100.0])[:Cc]
    vals[1, Cc:] = torch.tensor([100.0, 20.0, -30.0, -100.0])[:Cc]
    vals[:2, :Cc][vals[:2, Cc:] <= -30.0] = 0.0                       # no mean on the pixels at the lower clamp: exp(-15) eps alone
    vals = vals.to(DT[dn])
    eps = torch.randn(B, Cc, HW, generator=g)
    ref = _latent_ref(vals, eps, B, Cc, HW, 0.18215)
    logvar = vals.float().view(B, HW, 2 * Cc)[..., Cc:].permute(0, 2, 1)
    # three blocks, each against a scale of its own: everything (the pixels at the upper clamp, e^10 eps, set that scale), the
    # pixels below the upper clamp (the formula at ordinary values), and the mean-free pixels at the lower clamp (without the
    # clamp logvar = -100 gives e^-50 where e^-15 is due)
    blocks = (("all", torch.ones_like(logvar, dtype=torch.bool)), ("ordinary", logvar < 20.0), ("low_clamp", logvar <= -30.0))
    assert [int(m.sum()) for _, m in blocks] == [B * Cc * HW, B * Cc * HW - (4 if Cc == 4 else 3), 4 if Cc == 4 else 3]

    def errs(z):
        e = (z.double().view(B, Cc, HW) - ref).abs()
        return [float(e[m].max()) / (float(ref[m].abs().max()) + 1e-30) for _, m in blocks]

    z32 = (vals.float().view(B, HW, 2 * Cc)[..., :Cc].permute(0, 2, 1) + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * eps) * 0.18215
    assert max(errs(z32)) <= 1e-5 / 2, "fixture: fp32 on the CPU is within half the bound"
    unclamped = (vals.float().view(B, HW, 2 * Cc)[..., :Cc].permute(0, 2, 1) + torch.exp(0.5 * logvar.clamp(max=20.0)) * eps) * 0.18215
    assert errs(unclamped)[2] > 0.5, "fixture: the lower clamp shows in its block"
    mbuf, _ = _in_rows(vals.to(dev), ld)
    zbuf, z = _guarded(B * Cc * HW, dev, torch.float32)
    k.latent_sample(mbuf, eps.to(dev), z, B, Cc, HW, ld, 0.18215)
    what = f"B={B} C={Cc} HW={HW} ld={ld}"
    for (name, _), err in zip(blocks, errs(z.cpu())):
        _parity("latent_sample_" + name, dn, what, err, 1e-5)
    _guards_intact(zbuf, z.numel(), "latent_sample " + what)
    with pytest.raises(k.PdmkError):                                  # ld < 2 C
        k.latent_sample(mbuf, eps.to(dev), z, B, Cc, HW, 2 * Cc - 1, 0.18215)


@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
def test_latent_sample_large_exact(dev, dn):
    """logvar = 0 (exp(0) is exactly 1), integer means and noise, scale = 1/4: exact multiples of 1/4"""
    from pdm import _pdmk as k
    p = _large("latent_sample", dn)
    B, Cc, HW, ld = p["B"], p["C"], p["HW"], p["ld"]
    torch.manual_seed(HW)
    vals = _ints((B * HW, 2 * Cc), dev, DT[dn])
    vals[:, Cc:] = 0
    mbuf, _ = _in_rows(vals, ld)
    eps = _ints((B, Cc, HW), dev, torch.float32)
    zbuf, z = _guarded(B * Cc * HW, dev, torch.float32)
    k.latent_sample(mbuf, eps, z, B, Cc, HW, ld, 0.25)
    ref = (vals[:, :Cc].double().view(B, HW, Cc).permute(0, 2, 1) + eps.double()) * 0.25
    assert torch.equal(z.view(B, Cc, HW), ref.float()), f"latent_sample {dn} {_id(p)}"
    _guards_intact(zbuf, z.numel(), f"latent_sample {dn} {_id(p)}")


# ------------------------------------------------------------------------------------------------ token embedding
def _embed_case(dev, dn, B, T, D, vocab, pad, ids=None):
    """pad = (token, position, out) row padding in chunks.  The position table has a row for every output row and three more:
    rows past T hold other values than the rows the kernel must wrap to."""
    from pdm import _pdmk as k
    dt, v = DT[dn], V[dn]
    ntok = B * T
    ldt, ldp, ldo = (D + c * v for c in pad)
    tbuf, tok = _in_rows(_ints((vocab, D), dev, dt), ldt)
    pbuf, pos = _in_rows(_ints((ntok + 3, D), dev, dt), ldp)
    if ids is None:
        ids = torch.randint(0, vocab, (ntok,), device=dev)
    obuf, out = _out_rows(ntok, D, ldo, dev, dt)
    k.embed_tokens(ids, tbuf, pbuf, obuf, ntok, T, D, vocab, ldt, ldp, ldo)
    rows = torch.arange(ntok, device=dev)
    ref = (tok[ids.clamp(0, vocab - 1)].double() + pos[rows % T].double()).to(dt)
    what = f"embed_tokens {dn} B={B} T={T} D={D} vocab={vocab} pad={pad}"
    assert torch.equal(out, ref), what
    _pads_intact(obuf, ntok, D, what)


@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
def test_embed_tokens_exact(dev, dn):
    """One chunk per row and D = 64, dense and padded rows, a position table longer than T, vocab = 1, clamped ids"""
    torch.manual_seed(7)
    v = V[dn]
    for D in (v, 64):
        for pad in ((0, 0, 0), (1, 2, 3)):
            _embed_case(dev, dn, 5, 7, D, 11, pad)
        _embed_case(dev, dn, 1, 1, D, 11, (1, 2, 3))
        _embed_case(dev, dn, 2, 3, D, 1, (1, 0, 2))                                                  # vocab = 1
        ids = torch.tensor([-2 ** 40, 2 ** 40, -1, 11, 0, 10, 2 ** 31, -2 ** 31 - 1, 2 ** 32 + 3, 5], device=dev)
        _embed_case(dev, dn, 2, 5, D, 11, (1, 2, 3), ids=ids)                                        # clamped to [0, vocab)
        _embed_case(dev, dn, 2, 5, D, 1, (1, 2, 3), ids=ids)


@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
def test_embed_tokens_large(dev, dn):
    p = _large("embed_tokens", dn)
    torch.manual_seed(p["B"])
    _embed_case(dev, dn, p["B"], p["T"], p["D"], p["vocab"], (1, 1, 1))


# ------------------------------------------------------------------------------------------------ ViT patch embedding operands
def _im2col_case(dev, dn, B, S, p, ldo):
    from pdm import _pdmk as k
    G, K = S // p, 3 * p * p
    x = _ints((B, 3, S, S), dev, torch.float32, -128, 128)
    obuf = torch.full((B * G * G + ROWS_AFTER, ldo), SENT, device=dev, dtype=DT[dn])
    k.patch_im2col(x, obuf[:B * G * G], B, S, p)
    ref = x.view(B, 3, G, p, G, p).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, K)
    what = f"im2col {dn} B={B} S={S} p={p} ldo={ldo}"
    assert torch.equal(obuf[:B * G * G, :K], ref.to(DT[dn])), what
    assert bool((obuf[:B * G * G, K:] == 0).all()), what + ": the padding columns are zero-filled"
    assert bool((obuf[B * G * G:] == SENT).all()), what + ": rows after the last written"


@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
@pytest.mark.parametrize("S,p", [(28, 14), (32, 32), (64, 16)])
def test_patch_im2col_exact(dev, dn, S, p):
    torch.manual_seed(S)
    for ldo in (3 * p * p, 3 * p * p + 8):
        _im2col_case(dev, dn, 2, S, p, ldo)


@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
def test_patch_im2col_large(dev, dn):
    p = _large("im2col", dn)
    torch.manual_seed(p["B"])
    _im2col_case(dev, dn, p["B"], p["S"], p["p"], p["ldo"])


def _vit_case(dev, dn, B, G2, E):
    from pdm import _pdmk as k
    dt = DT[dn]
    ldp, ldpos, ldo = E + 3, E + 5, E + 8
    pbuf, patches = _in_rows(_ints((B * G2, E), dev, dt), ldp)
    cbuf, cls = _in_rows(_ints((1, E), dev, dt), E + 7)
    qbuf, pos = _in_rows(_ints((G2 + 1, E), dev, dt), ldpos)
    obuf, out = _out_rows(B * (G2 + 1), E, ldo, dev, dt)
    k.vit_tokens(pbuf, cbuf, qbuf, ldpos, obuf, B, G2, E)
    ref = torch.cat([cls.double().expand(B, 1, E), patches.double().view(B, G2, E)], 1) + pos.double()
    what = f"vit_tokens {dn} B={B} G2={G2} E={E}"
    assert torch.equal(out, ref.view(B * (G2 + 1), E).to(dt)), what
    _pads_intact(obuf, B * (G2 + 1), E, what)


@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
@pytest.mark.parametrize("shape", [(1, 4, 5), (3, 4, 5), (1, 16, 96), (3, 16, 96), (2, 1, 96), "large"], ids=str)
def test_vit_tokens_exact(dev, dn, shape):
    if shape == "large":
        p = _large("vit_tokens", dn)
        shape = p["B"], p["G2"], p["E"]
    B, G2, E = shape
    torch.manual_seed(B + E)
    _vit_case(dev, dn, B, G2, E)


# ------------------------------------------------------------------------------------------------ QuickGELU
@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
@pytest.mark.parametrize("n", GELU_N + ("large",))
def test_quick_gelu_forms(dev, dn, n):
    from pdm import _pdmk as k
    n = _large("quick_gelu", dn)["n"] if n == "large" else n
    x, ref = _gelu_case(n, dn)
    y32 = (x.float() * torch.sigmoid(1.702 * x.float())).to(DT[dn])
    assert max(_gelu_errs(y32, ref)) <= GELU_TOL[dn] / 2, "fixture: fp32 on the CPU is within half the bound"
    xd = x.to(dev)
    ybuf, y = _guarded(n, dev, DT[dn])
    k.quick_gelu_fwd(xd, y)
    for part, err in zip(("all", "random"), _gelu_errs(y.cpu(), ref)):
        _parity("quick_gelu_" + part, dn, f"n={n}", err, GELU_TOL[dn])
    _guards_intact(ybuf, n, f"quick_gelu {dn} n={n}")
    if n > CAPS["quick_gelu"] * NT:         # the same elements through launches that fit in one pass
        L = 1000000
        assert -(-L // NT) < CAPS["quick_gelu"]
        y2buf, y2 = _guarded(n, dev, DT[dn])
        for lo in range(0, n, L):
            k.quick_gelu_fwd(xd[lo:lo + L], y2[lo:lo + L])
        assert torch.equal(y, y2), f"quick_gelu {dn}: the looping launch differs from one-pass launches over slices"
        _guards_intact(y2buf, n, f"quick_gelu {dn} slices")


# ------------------------------------------------------------------------------------------------ pooled rows
@pytest.mark.gpu
@pytest.mark.parametrize("dn", BOTH)
@pytest.mark.parametrize("D", [1, 256, 257, 768])
@pytest.mark.parametrize("B,T", [(1, 1), (5, 77), (1, 77), (5, 1)])
def test_gather_rows_moves(dev, dn, D, B, T):
    """A pure move: the row at the first maximum of the ids (at position 0, at T - 1, repeated, all ids negative), or row 0"""
    from pdm import _pdmk as k
    dt = DT[dn]
    torch.manual_seed(D + B + T)
    ldx, ldo = D + 5, D + 3
    xbuf, x = _in_rows(torch.randn(B * T, D, device=dev).to(dt), ldx)
    xv = x.reshape(B, T, D)
    patterns = []
    base = torch.randint(0, 1000, (B, T))
    for kind in ("first", "last", "repeated", "negative"):
        ids = base.clone()
        if kind == "first":
            ids[:, 0] = 49407
        elif kind == "last":
            ids[:, T - 1] = 49407
        elif kind == "repeated":
            ids[:, T // 3] = 49407
            ids[:, T - 1] = 49407
            ids[:, (2 * T) // 3] = 49407
        else:
            ids = -ids - 5
            ids[:, T // 2] = -2
            ids[:, T - 1] = -2
        patterns.append((kind, ids))
    for kind, ids in patterns:
        first = torch.tensor([int((r == r.max()).nonzero()[0]) for r in ids])
        if kind == "first":
            assert bool((first == 0).all())
        elif kind == "last":
            assert bool((first == T - 1).all())
        else:
            assert bool((first == (T // 3 if kind == "repeated" else T // 2)).all())
        obuf, out = _out_rows(B, D, ldo, dev, dt)
        k.gather_rows(xbuf, ids.to(dev), T, obuf, B, D)
        what = f"gather_rows {dn} D={D} B={B} T={T} {kind}"
        assert torch.equal(out, xv[torch.arange(B, device=dev), first.to(dev)]), what
        _pads_intact(obuf, B, D, what)
    obuf, out = _out_rows(B, D, ldo, dev, dt)
    k.gather_rows(xbuf, None, T, obuf, B, D)
    assert torch.equal(out, xv[:, 0]), f"gather_rows {dn} D={D} B={B} T={T} ids=None"
    _pads_intact(obuf, B, D, "gather_rows ids=None")


# ------------------------------------------------------------------------------------------------ score head
HEAD_MODES = ("a_only", "all", "acc_only", "no_acc")
ACC0 = 0.25


def _head_run(dev, a, b, mode):
    """Run one pointer mode on CPU fp32 rows a, b [B, D] (strided on the device, 1e6 in the padding).  Returns (an, bn, acc
    increment), None where the mode does not ask for it; checks that whatever was not requested, and rows past B, kept their
    sentinels."""
    from pdm import _pdmk as k
    B, D = a.shape
    abuf, _ = _in_rows(a.to(dev), D + 5)
    bbuf, _ = _in_rows(b.to(dev), D + 9)
    anbuf, an = _out_rows(B, D, D, dev, torch.float32)
    bnbuf, bn = _out_rows(B, D, D, dev, torch.float32)
    accbuf = torch.tensor([SENT, ACC0, SENT], device=dev, dtype=torch.float64)
    acc = accbuf[1:2]
    want_an, want_b, want_bn, want_acc = {"a_only": (1, 0, 0, 0), "all": (1, 1, 1, 1), "acc_only": (0, 1, 0, 1),
                                          "no_acc": (1, 1, 1, 0)}[mode]
    rc = k._lib.pdmk_clip_score_head(k._p(abuf), D + 5, k._p(bbuf) if want_b else None, D + 9 if want_b else 0,
                                     k._p(anbuf) if want_an else None, k._p(bnbuf) if want_bn else None,
                                     k._p(acc) if want_acc else None, B, D, k._st())
    assert rc == 0, mode
    what = f"clip_score_head B={B} D={D} {mode}"
    for buf, want in ((anbuf, want_an), (bnbuf, want_bn)):
        assert bool((buf[B:] == SENT).all()), what + ": rows past B written"
        assert want or bool((buf == SENT).all()), what + ": an output that was not requested was written"
    got = accbuf.cpu().tolist()
    assert got[0] == SENT and got[2] == SENT and (want_acc or got[1] == ACC0), what + f": acc = {got}"
    return (an.cpu() if want_an else None), (bn.cpu() if want_bn else None), (got[1] - ACC0 if want_acc else None)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", HEAD_MODES)
@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("D", [1, 64, 255, 256, 257, 768, 1000])
def test_clip_score_head_modes(dev, D, B, mode):
    """fp64 normalisation: an, bn at 1e-6 of their scale, the accumulator's increment at 1e-5 per cosine"""
    g = torch.Generator().manual_seed(D * 8 + B)
    a = torch.randn(B, D, generator=g)
    b = torch.randn(B, D, generator=g) + 0.5 * a
    ra = a.double() / a.double().norm(dim=1, keepdim=True)
    rb = b.double() / b.double().norm(dim=1, keepdim=True)
    an, bn, inc = _head_run(dev, a, b, mode)
    what = f"B={B} D={D} {mode}"
    if an is not None:
        _parity("score_head_an", "f32", what, float((an.double() - ra).abs().max()) / (float(ra.abs().max()) + 1e-6), 1e-6)
    if bn is not None:
        _parity("score_head_bn", "f32", what, float((bn.double() - rb).abs().max()) / (float(rb.abs().max()) + 1e-6), 1e-6)
    if inc is not None:
        _parity("score_head_acc", "f32", what, abs(inc - float((ra * rb).sum())), COS_TOL * B)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", HEAD_MODES)
@pytest.mark.parametrize("D", [256, 257, 768, 1000])
def test_clip_score_head_exact(dev, D, mode):
    """Rows of 0 / +-1 with exactly 256 non-zeros, columns 255, 256 and D - 1 among them: every norm is 16, an and bn are
    +-1/16 or 0, every dot product a multiple of 1/256; an, bn and the accumulator's increment are exact"""
    B = 7
    g = torch.Generator().manual_seed(D)
    rows = []
    for _ in range(2 * B):
        must = sorted({255, min(256, D - 1), D - 1})
        rest = [c for c in torch.randperm(D, generator=g).tolist() if c not in must][:256 - len(must)]
        r = torch.zeros(D)
        idx = torch.tensor(must + rest)
        r[idx] = torch.randint(0, 2, (256,), generator=g).float() * 2 - 1
        assert int((r != 0).sum()) == 256
        rows.append(r)
    a, b = torch.stack(rows[:B]), torch.stack(rows[B:])
    an, bn, inc = _head_run(dev, a, b, mode)
    what = f"D={D} {mode}"
    if an is not None:
        assert torch.equal(an, a / 16), what + " an"
    if bn is not None:
        assert torch.equal(bn, b / 16), what + " bn"
    if inc is not None:
        assert inc == float((a.double() * b.double()).sum()) / 256, what + " acc"


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refused_calls_leave_outputs_untouched(dev):
    """The argument checks of the family, one argument off a call that is accepted: status -1, and nothing written"""
    from pdm import _pdmk as k
    torch.manual_seed(9)
    outs = []

    def out(n, dt=torch.float32):
        t = torch.full((n,), SENT, device=dev, dtype=dt)
        outs.append(t)
        return t

    def refused(fn, *a, **kw):
        with pytest.raises(k.PdmkError):
            fn(*a, **kw)

    fl = _ints((4096,), dev, torch.float32)
    bf = _ints((4096,), dev, torch.bfloat16)
    # softmax: cols & 3, lds & 3, lds < cols, ldp < cols, misaligned s, cols past the widest form
    k.softmax_rows(fl, torch.empty(64, device=dev), 2, 8, 12, 9)
    refused(k.softmax_rows, fl, out(64), 2, 6, 12, 9)
    refused(k.softmax_rows, fl, out(64), 2, 8, 14, 9)
    refused(k.softmax_rows, fl, out(64), 2, 8, 4, 9)
    refused(k.softmax_rows, fl, out(64), 2, 8, 12, 7)
    refused(k.softmax_rows, fl[1:], out(64), 2, 8, 12, 9)
    refused(k.softmax_rows, fl, out(64, torch.bfloat16), 2, 8, 12, 7)
    wide = torch.zeros(SOFTMAX_MAX + 4, device=dev)
    refused(k.softmax_rows, wide, out(SOFTMAX_MAX + 4), 1, SOFTMAX_MAX + 4, SOFTMAX_MAX + 4, SOFTMAX_MAX + 4)
    refused(k.softmax_rows, wide, out(SOFTMAX_MAX + 4, torch.bfloat16), 1, SOFTMAX_MAX + 4, SOFTMAX_MAX + 4, SOFTMAX_MAX + 4)
    # embed_tokens: D, ldt, ldp, ldo not a multiple of the chunk; misaligned tok, pos, out
    ids = torch.zeros(4, dtype=torch.int64, device=dev)
    for src, dt, v in ((bf, torch.bfloat16, 8), (fl, torch.float32, 4)):
        k.embed_tokens(ids, src, src, torch.empty(256, device=dev, dtype=dt), 4, 2, 2 * v, 3, 3 * v, 3 * v, 3 * v)
        h = v // 2
        refused(k.embed_tokens, ids, src, src, out(256, dt), 4, 2, 2 * v - h, 3, 3 * v, 3 * v, 3 * v)
        refused(k.embed_tokens, ids, src, src, out(256, dt), 4, 2, 2 * v, 3, 3 * v + h, 3 * v, 3 * v)
        refused(k.embed_tokens, ids, src, src, out(256, dt), 4, 2, 2 * v, 3, 3 * v, 3 * v + h, 3 * v)
        refused(k.embed_tokens, ids, src, src, out(256, dt), 4, 2, 2 * v, 3, 3 * v, 3 * v, 3 * v + h)
        refused(k.embed_tokens, ids, src[1:], src, out(256, dt), 4, 2, 2 * v, 3, 3 * v, 3 * v, 3 * v)
        refused(k.embed_tokens, ids, src, src[1:], out(256, dt), 4, 2, 2 * v, 3, 3 * v, 3 * v, 3 * v)
        refused(k.embed_tokens, ids, src, src, out(257, dt)[1:], 4, 2, 2 * v, 3, 3 * v, 3 * v, 3 * v)
        refused(k.embed_tokens, ids, src, src, out(256, dt), 4, 2, 2 * v, 0, 3 * v, 3 * v, 3 * v)
    # im2col: S not a multiple of p, ldo < K
    x = _ints((1, 3, 9, 9), dev, torch.float32)
    raw = lambda S, p, ldo, o: k._lib.pdmk_patch_im2col(k._p(x), k._p(o), 1, S, p, ldo, k.F32, k._st())      # noqa: E731
    assert raw(8, 4, 48, torch.empty(4 * 48, device=dev)) == 0
    assert raw(9, 4, 48, out(4 * 48 + 64)) == -1 and raw(8, 4, 47, out(4 * 48)) == -1 and raw(2, 4, 48, out(4 * 48)) == -1
    # vit_tokens: a row stride below E; gather_rows: ldx or ldo below D
    rawv = lambda ldp, ldpos, ldo: k._lib.pdmk_vit_tokens(k._p(fl), ldp, k._p(fl), k._p(fl), ldpos, k._p(out(256)), ldo, 2, 3, 8,      # noqa: E731
                                                          k.F32, k._st())
    assert rawv(7, 8, 8) == -1 and rawv(8, 7, 8) == -1 and rawv(8, 8, 7) == -1
    rawg = lambda ldx, ldo: k._lib.pdmk_gather_rows(k._p(fl), ldx, None, 3, k._p(out(64)), ldo, 2, 8, k.F32, k._st())      # noqa: E731
    assert rawg(7, 8) == -1 and rawg(8, 7) == -1
    # score head: lda < D, ldb < D, b = None with bn or acc set, an = None with b = None
    acc = torch.full((1,), 3.0, device=dev, dtype=torch.float64)
    rawh = lambda lda, b, ldb, an, bn, ac: k._lib.pdmk_clip_score_head(k._p(fl), lda, k._p(b), ldb, k._p(an), k._p(bn), k._p(ac), 2, 8,      # noqa: E731
                                                                       k._st())
    assert rawh(8, fl, 8, torch.empty(16, device=dev), torch.empty(16, device=dev), None) == 0
    assert rawh(7, fl, 8, out(16), out(16), acc) == -1 and rawh(8, fl, 7, out(16), out(16), acc) == -1
    assert rawh(8, None, 0, out(16), out(16), None) == -1 and rawh(8, None, 0, out(16), None, acc) == -1
    assert rawh(8, None, 0, None, None, None) == -1
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENT).all()), "a refused call wrote its output"
    assert acc.item() == 3.0
