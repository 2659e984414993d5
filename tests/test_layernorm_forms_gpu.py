"""LayerNorm backward (pdmk_layernorm_bwd): every lane-group form of the kernel, ragged rows and columns, strided operands,
the `add` / accumulate_dx operand forms and the deferred partial slabs, against fp64 torch.

The kernel gives a row to a group of L lanes with S 16-byte chunks per lane (csrc/norm.hip, ln_bwd_form); FORMS below says
which (L, S) each (dtype, C) of the tests reaches and `_form` restates the dispatch rule, so that the table can be checked to
reach every instantiation.  The reference is computed in fp64 from the rounded inputs and from the (mean, rstd) array handed to
the kernel - that array is built here, so the backward is tested independently of the forward.

Bit-reproducibility: dx and the per-block slabs (what this kernel writes: plain stores, fixed summation order) are compared
bit for bit between two runs.  dgamma / dbeta come out of the second stage (reduce_partials_kernel), which adds up to 8 slice
sums per address with fp32 atomics once there are 32 slabs or more, so their last bit follows the arrival order there; they
are compared bit for bit where the second stage has one slice (fewer than 32 blocks)."""
import ctypes as C

import pytest
import torch

from test_kernels_gpu import DT, TOL, close

V = {"bf16": 8, "f32": 4}
# (dtype, C) -> (L, S); 328 (bf16) and 164 (f32) leave a ragged last slot, 2560 (bf16) and 1280 (f32) reach the 320-chunk limit,
# 24 (bf16) and 8 (f32) are rows of fewer chunks than the smallest lane group
FORMS = {
    ("bf16", 24): (8, 1), ("f32", 8): (8, 1),
    ("bf16", 64): (8, 1), ("bf16", 128): (8, 2), ("bf16", 192): (8, 3), ("bf16", 320): (16, 3), ("bf16", 328): (16, 3),
    ("bf16", 640): (32, 3), ("bf16", 1280): (64, 3), ("bf16", 2560): (64, 5),
    ("f32", 32): (8, 1), ("f32", 64): (8, 2), ("f32", 96): (8, 3), ("f32", 160): (16, 3), ("f32", 164): (16, 3),
    ("f32", 320): (32, 3), ("f32", 640): (64, 3), ("f32", 1280): (64, 5),
}
ALL_FORMS = {(8, 1), (8, 2), (8, 3), (16, 3), (32, 3), (64, 3), (64, 5)}


def _form(nchunks):
    """ln_bwd_form of csrc/norm.hip"""
    for lim, f in ((8, (8, 1)), (16, (8, 2)), (24, (8, 3)), (48, (16, 3)), (96, (32, 3)), (192, (64, 3))):
        if nchunks <= lim:
            return f
    return (64, 5)


def _rows_per_blk(M):
    """ln_bwd_rows_per_blk of csrc/norm.hip"""
    rpb = (M + 511) // 512
    if rpb <= 16:
        return 16
    return 256 if rpb > 224 else (rpb + 31) // 32 * 32


def _cases():
    out = []
    for (dn, Cc), (L, S) in FORMS.items():
        for M in sorted({1, max(1, 64 // L - 1), 53, 300}):       # 300 rows: 19 blocks of 16, the last one ragged
            out.append((dn, Cc, M))
    # the two ends of the grid rule above its floor of 16 rows per block: 64 rows (the step's largest LayerNorm, 512 blocks)
    # and the cap of 256 rows (ragged: 513 blocks)
    out.append(("bf16", 320, 32768))
    out.append(("bf16", 64, 131077))
    return out


def test_form_table_reaches_every_instantiation():
    for dn in ("bf16", "f32"):
        assert {f for (d, _), f in FORMS.items() if d == dn} == ALL_FORMS
    for (dn, Cc), f in FORMS.items():
        assert Cc % V[dn] == 0 and _form(Cc // V[dn]) == f, (dn, Cc)
    assert {_form(n) for n in range(1, 321)} == ALL_FORMS
    assert _rows_per_blk(32768) == 64 and _rows_per_blk(131077) == 256 and _rows_per_blk(300) == 16


def test_partial_dims_fit_the_promised_workspace():
    """Host only: the slab count of every grid the rule produces fits what pdmk.h promises ((M / 16 + 1) * 2 * C floats)."""
    from pdm import _pdmk as k
    for M in (1, 15, 16, 17, 512, 2048, 8192, 32768, 65536, 70001):
        for Cc in (64, 320, 640, 1280, 2560):
            nblk, n = k._dims(k._lib.pdmk_layernorm_bwd_partial_dims, M, Cc)
            assert nblk >= 1 and n == Cc, (M, Cc, nblk, n)
            assert nblk * 2 * n * 4 <= k._lib.pdmk_layernorm_bwd_part_workspace_bytes(M, Cc), (M, Cc, nblk)
            assert nblk == (M + _rows_per_blk(M) - 1) // _rows_per_blk(M), (M, nblk)
    assert k._dims(k._lib.pdmk_layernorm_bwd_partial_dims, 8192, 640) == (512, 640)
    assert k._dims(k._lib.pdmk_layernorm_bwd_partial_dims, 2048, 1280) == (128, 1280)
    assert k._dims(k._lib.pdmk_layernorm_bwd_partial_dims, 512, 1280) == (32, 1280)
    assert k._dims(k._lib.pdmk_layernorm_bwd_partial_dims, 65536, 320) == (512, 320)


PAD, ROWS_AFTER, SENT = 8, 3, 7.0


def _view(buf, M, Cc):
    return buf[:M, PAD:PAD + Cc]


def _strided(M, Cc, dev, dt, fill=None):
    """[M, Cc] view with row stride Cc + 16 that starts 8 columns into its buffer; ROWS_AFTER rows follow it."""
    if fill is None:
        buf = torch.randn(M + ROWS_AFTER, Cc + 2 * PAD, device=dev).to(dt)
    else:
        buf = torch.full((M + ROWS_AFTER, Cc + 2 * PAD), fill, device=dev, dtype=dt)
    return buf, _view(buf, M, Cc)


def _sentinels_intact(buf, M, Cc, what):
    assert bool((buf[:, :PAD] == SENT).all()) and bool((buf[:, PAD + Cc:] == SENT).all()), f"{what}: columns beside dx written"
    assert bool((buf[M:] == SENT).all()), f"{what}: rows after M written"


@pytest.mark.gpu
@pytest.mark.parametrize("dn,Cc,M", _cases())
def test_layernorm_bwd_forms(dev, dn, Cc, M):
    from pdm import _pdmk as k
    torch.manual_seed(1000 * Cc + M)
    dt = DT[dn]
    ld = Cc + 2 * PAD
    # every row has its own offset and scale, gamma is distinct per column: a row or a column taken for another shows
    mu = torch.linspace(-3, 3, M, device=dev)[torch.randperm(M, device=dev)]
    sd = torch.linspace(0.1, 4, M, device=dev)[torch.randperm(M, device=dev)]
    xbuf, x = _strided(M, Cc, dev, dt)
    x.copy_((torch.randn(M, Cc, device=dev) * sd[:, None] + mu[:, None]).to(dt))
    dybuf, dy = _strided(M, Cc, dev, dt)
    addbuf, add = _strided(M, Cc, dev, dt)
    gamma = (0.5 + torch.arange(Cc, device=dev) / Cc + 0.01 * torch.randn(Cc, device=dev)).float()
    xd = x.double()
    mean = xd.mean(1)
    rstd = (xd.var(1, unbiased=False) + 1e-5).rsqrt()
    stats = torch.stack([mean, rstd], 1).float().contiguous()
    # fp64 reference from the rounded inputs and the fp32 statistics the kernel reads
    m64, r64 = stats[:, 0:1].double(), stats[:, 1:2].double()
    h = (xd - m64) * r64
    g = dy.double() * gamma.double()
    ref_dx = r64 * (g - g.mean(1, keepdim=True) - h * (g * h).mean(1, keepdim=True))
    ref_dg, ref_db = (dy.double() * h).sum(0), dy.double().sum(0)
    base = torch.randn(M, Cc, device=dev).to(dt)
    nblk, n = k._dims(k._lib.pdmk_layernorm_bwd_partial_dims, M, Cc)
    assert n == Cc and nblk == (M + _rows_per_blk(M) - 1) // _rows_per_blk(M)

    def run(acc, with_add):
        dxbuf, dx = _strided(M, Cc, dev, dt, fill=SENT)
        if acc:
            dx.copy_(base)
        dg, db = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
        k.layernorm_bwd(x, dy, dx, gamma, stats, dg, db, M, Cc, ld, ld, ld, acc, add=add if with_add else None)
        return dxbuf, dx, dg, db

    direct = None
    for acc in (False, True):
        for with_add in (False, True):
            what = f"{dn} {M}x{Cc} acc={acc} add={with_add}"
            dxbuf, dx, dg, db = run(acc, with_add)
            ref = ref_dx + (base.double() if acc else 0.0) + (add.double() if with_add else 0.0)
            close(dx, ref, TOL[dn] * 2, what + " dx")
            close(dg, ref_dg, TOL[dn] * 2, what + " dgamma")
            close(db, ref_db, TOL[dn] * 2, what + " dbeta")
            _sentinels_intact(dxbuf, M, Cc, what)
            _, dx2, dg2, db2 = run(acc, with_add)
            assert torch.equal(dx, dx2), what + ": dx differs between two runs"
            if nblk < 32:       # one slice in the second stage: no atomics meet (module docstring)
                assert torch.equal(dg, dg2) and torch.equal(db, db2), what + ": dgamma / dbeta differ between two runs"
            if not acc and not with_add:
                direct = (dx, dg, db)

    # deferred form through the C entry point: dgamma = dbeta = NULL, part_ws exactly nblk * 2 * n floats
    slabs = []
    for rep in range(2):
        pbuf = torch.full((nblk * 2 * n + 64,), -123.0, device=dev)
        part = pbuf[32:32 + nblk * 2 * n]
        dxbuf, dx = _strided(M, Cc, dev, dt, fill=SENT)
        rc = k._lib.pdmk_layernorm_bwd(k._p(x), k._p(dy), k._p(dx), k._p(gamma), k._p(stats), None, None, k._p(part),
                                       part.numel(), M, Cc, ld, ld, ld, 0, None, 0, k.dt(x), k._st())
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((pbuf[:32] == -123.0).all()) and bool((pbuf[32 + nblk * 2 * n:] == -123.0).all()), "slab overrun"
        assert torch.equal(dx, direct[0])
        _sentinels_intact(dxbuf, M, Cc, "deferred")
        slabs.append((pbuf, part))
    assert torch.equal(slabs[0][1], slabs[1][1]), "partial slabs differ between two runs"
    # one float short: refused, nothing launched
    assert k._lib.pdmk_layernorm_bwd(k._p(x), k._p(dy), k._p(dx), k._p(gamma), k._p(stats), None, None, k._p(part),
                                     part.numel() - 1, M, Cc, ld, ld, ld, 0, None, 0, k.dt(x), k._st()) == -1
    dg, db = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
    item = (k.PartialItem * 1)()
    item[0].part, item[0].out0, item[0].out1, item[0].nblk, item[0].n = k._p(part), k._p(dg), k._p(db), nblk, n
    assert k._lib.pdmk_reduce_partials_group(C.cast(item, C.c_void_p), 1, k._st()) == 0
    torch.cuda.synchronize()
    for a, b in ((dg, direct[1]), (db, direct[2])):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max() + 1e-6), "deferred reduction differs from the direct form"
    assert bool((slabs[1][0][:32] == -123.0).all()) and bool((slabs[1][0][32 + nblk * 2 * n:] == -123.0).all())
