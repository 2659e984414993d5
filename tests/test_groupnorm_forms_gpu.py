"""GroupNorm forward and backward (pdmk_groupnorm_fwd / pdmk_groupnorm_bwd): every thread-map form and grid form of the four
kernels, distinct statistics per (image, group), strided operands, the `add` / accumulate_dx operand forms, padding channels,
unaligned gamma / beta and the cancellation the double-precision variance guards against, against fp64 torch.

A block gives tpr = min(C / V, 256) threads to a row and keeps rif = 256 / tpr rows in flight; a thread owns
slots = ceil(C / V / 256) 16-byte chunks of its row (csrc/norm.hip, gn_map2 and gn_fwd / gn_bwd).  FORMS below says which
(tpr, rif, slots) each (dtype, C) of the tests reaches and with which group layout and (B, HW) it runs; `_map2`, `_slots` and
`_rows_per_blk` restate the dispatch and grid rules, so that the table can be checked to reach every form on a machine without
a GPU.

Reference: fp64 torch on the rounded inputs, written out plainly - per-(image, group) mean and biased variance,
rstd = (var + eps)^-1/2, z = xhat * gamma + beta, optional SiLU, the backward through torch.autograd.grad.  The backward gets a
(mean, rstd) array built here from that reference and rounded to fp32, so it is tested independently of the forward.

Inputs: x[b, :, group g] = sigma[b, g] * (n + u[b, g]) with sigma log-uniform in [0.25, 4], u uniform in [-3, 3] and n normal
noise that is standardised per (image, group) - exactly zero mean and unit variance over the group's HW * gs cells - so that
|mean| / std = |u| <= 3 holds for every group whatever its size (with a handful of cells the sample variance of plain randn can
come out tiny, and then E[x^2] - mean^2 of fp32 sums says nothing about the kernel).  For the same reason every case has at
least 4 cells per group: dx of a group of n cells has n - 2 degrees of freedom, and is identically zero at n = 2.

Comparisons are per (image, group) block - max |got - ref| <= tol * max |ref| over that block - so that a group of small scale
cannot hide behind a large one; dgamma / dbeta per group.  Each comparison prints a GN_PARITY line before it asserts
(profiles/groupnorm_parity.txt is a collected run).  GN_DIGEST lines print the sha256 of y (its whole buffer), stats, dx (whole
buffer) and the single-slice dgamma / dbeta: two builds of the library compute the same bits if their runs print the same lines
(profiles/gn_refactor_digest.txt).

Bit-reproducibility: y, stats and dx are plain stores in a fixed order and are compared bit for bit between two runs.
dgamma / dbeta come out of the second stage (launch_reduce_partials -> reduce_partials_kernel), which splits the nblk slabs of
the backward statistics pass (all images' blocks) into 4 slices from 32 slabs and 8 from 256, one fp32 atomic per slice and
address: their last bit follows the arrival order there, so they are compared bit for bit where nblk < 32 (one slice)."""
import ctypes as C
import math

import pytest
import torch

from test_kernels_gpu import DT, TOL, close, digest  # noqa: F401  (close: the project's whole-tensor check, used for the slab form)

NT = 256
V = {"bf16": 8, "f32": 4}
EPS = 1e-5

# (dtype, C) -> ((tpr, rif, slots), (G, gs), ((B, HW), ...))
# bf16: 176 / G*gs 170 and 40 / 34 have padding channels and a chunk that straddles the last group's end; 2056 = 8 * 257 and
# 4104 = 54 * 76 put the first ragged chunk of slots 2 and 3 inside a group; 128 and 4096 run 64 groups, 8 runs one.
FORMS = {
    ("bf16", 8): ((1, 256, 1), (1, 8), ((2, 1), (2, 255))),
    ("bf16", 40): ((5, 51, 1), (17, 2), ((2, 50),)),
    ("bf16", 128): ((16, 16, 1), (64, 2), ((2, 15),)),
    ("bf16", 176): ((22, 11, 1), (17, 10), ((2, 10), (3, 100))),
    ("bf16", 256): ((32, 8, 1), (32, 8), ((3, 20),)),
    ("bf16", 320): ((40, 6, 1), (32, 10), ((2, 1), (3, 1000), (1, 4096))),
    ("bf16", 512): ((64, 4, 1), (32, 16), ((2, 3),)),
    ("bf16", 640): ((80, 3, 1), (32, 20), ((2, 2),)),
    ("bf16", 960): ((120, 2, 1), (32, 30), ((2, 1),)),
    ("bf16", 1280): ((160, 1, 1), (32, 40), ((40, 16),)),
    ("bf16", 1920): ((240, 1, 1), (32, 60), ((2, 33),)),
    ("bf16", 2048): ((256, 1, 1), (32, 64), ((2, 17),)),
    ("bf16", 2056): ((256, 1, 2), (8, 257), ((2, 9),)),
    ("bf16", 2560): ((256, 1, 2), (32, 80), ((2, 64),)),
    ("bf16", 4096): ((256, 1, 2), (64, 64), ((2, 5),)),
    ("bf16", 4104): ((256, 1, 3), (54, 76), ((2, 12),)),
    ("bf16", 6144): ((256, 1, 3), (32, 192), ((2, 7),)),
    ("f32", 4): ((1, 256, 1), (1, 4), ((2, 1), (2, 255))),
    ("f32", 20): ((5, 51, 1), (17, 1), ((2, 50),)),
    ("f32", 88): ((22, 11, 1), (17, 5), ((2, 10), (3, 100))),
    ("f32", 128): ((32, 8, 1), (64, 2), ((2, 7),)),
    ("f32", 160): ((40, 6, 1), (32, 5), ((2, 1), (3, 1000), (1, 4096))),
    ("f32", 320): ((80, 3, 1), (32, 10), ((2, 2),)),
    ("f32", 640): ((160, 1, 1), (32, 20), ((40, 16),)),
    ("f32", 1024): ((256, 1, 1), (32, 32), ((2, 17),)),
    ("f32", 1028): ((256, 1, 2), (4, 257), ((2, 9),)),
    ("f32", 2048): ((256, 1, 2), (64, 32), ((2, 64),)),
    ("f32", 2052): ((256, 1, 3), (54, 38), ((2, 12),)),
    ("f32", 3072): ((256, 1, 3), (32, 96), ((2, 7),)),
}
MODEL_WIDTHS = (320, 640, 960, 1280, 1920, 2560, 128, 256, 512)      # U-Net and VAE channel widths, all bf16
# launch -> (rows of one sweep / rif, block target, blocks per image at most): gn_fwd and gn_bwd of csrc/norm.hip
LAUNCHES = {"fwd_stats": (8, 512, 64), "fwd_apply": (4, 1024, 1 << 20), "bwd_stats": (4, 512, 64), "bwd_apply": (2, 1024, 1 << 20)}


def _map2(nchunks):
    """gn_map2 of csrc/norm.hip"""
    tpr = min(nchunks, NT)
    return tpr, NT // tpr


def _slots(nchunks):
    return (nchunks + NT - 1) // NT


def _rows_per_blk(B, HW, sweep, target, max_blk):
    """gn_rows_per_blk of csrc/norm.hip"""
    nb = (target + B - 1) // B
    nb = max(1, min(nb, max_blk, HW // max(1, sweep)))
    rpb = (HW + nb - 1) // nb
    return (rpb + sweep - 1) // sweep * sweep


def _blocks(launch, B, HW, rif):
    """blocks per image of one of the four launches"""
    unr, target, max_blk = LAUNCHES[launch]
    rpb = _rows_per_blk(B, HW, rif * unr, target, max_blk)
    return (HW + rpb - 1) // rpb


def _slices(nblk):
    """launch_reduce_partials of csrc/norm.hip"""
    return 8 if nblk >= 256 else (4 if nblk >= 32 else 1)


def _cases():
    return [(dn, Cc, B, HW) for (dn, Cc), (_, _, shapes) in FORMS.items() for B, HW in shapes]


def test_form_table_reaches_every_form():
    """Host only: the table matches the restated rules and reaches every thread-map and grid form."""
    for (dn, Cc), ((tpr, rif, slots), (G, gs), shapes) in FORMS.items():
        assert Cc % V[dn] == 0 and G <= 64 and G * gs <= Cc, (dn, Cc)
        n = Cc // V[dn]
        assert _map2(n) == (tpr, rif) and _slots(n) == slots and n <= 3 * NT, (dn, Cc)
        for B, HW in shapes:
            assert HW * gs >= 4, (dn, Cc, HW)                      # module docstring: dx keeps n - 2 degrees of freedom
            assert B >= 2 or (B, HW) == (1, 4096), (dn, Cc, B)
            assert HW <= 64 or Cc < 1024, (dn, Cc, HW)
            assert (B * HW + 3) * (Cc + 16) * 8 <= 16 << 20        # the fp64 copy of the largest operand: a few MB
    for dn in ("bf16", "f32"):
        ent = {Cc: v for (d, Cc), v in FORMS.items() if d == dn}
        chunks = {Cc // V[dn] for Cc in ent}
        assert {v[0][2] for v in ent.values()} == {1, 2, 3}
        assert any(v[0][1] == 256 for v in ent.values()), "a single chunk"
        assert any(256 % v[0][0] for v in ent.values()), "a tpr that does not divide 256"
        assert any(129 <= c <= 255 for c in chunks), "rif = 1 with inactive threads"
        assert {256, 257, 512, 513, 768} <= chunks
        gl = {v[1] for v in ent.values()}
        assert any(G == 64 and gs == 2 for G, gs in gl) and any(G == 1 and gs == Cc for Cc, v in ent.items() for G, gs in [v[1]])
        assert any(G == 32 for G, _ in gl) and any(G == 17 for G, _ in gl)
        assert any(G * gs < Cc for Cc, v in ent.items() for G, gs in [v[1]]), "padding channels"
        shapes = {(Cc, B, HW) for Cc, v in ent.items() for B, HW in v[2]}
        rif_of = {Cc: v[0][1] for Cc, v in ent.items()}
        # one block per image: a single row, and one row short of a sweep of the narrowest launch
        assert any(HW == 1 for _, _, HW in shapes)
        assert any(HW == rif_of[Cc] - 1 and rif_of[Cc] > 2 for Cc, _, HW in shapes)
        for Cc, B, HW in shapes:
            if HW == 1 or HW == rif_of[Cc] - 1:
                assert all(_blocks(l, B, HW, rif_of[Cc]) == 1 for l in LAUNCHES), (dn, Cc, HW)
        c320 = 320 if dn == "bf16" else 160                          # 40 chunks in either dtype
        assert {(c320, 3, 1000), (c320, 1, 4096)} <= shapes and rif_of[c320] == 6
        # several blocks, the last one ragged, in all four launches
        for l, (unr, target, max_blk) in LAUNCHES.items():
            rpb = _rows_per_blk(3, 1000, 6 * unr, target, max_blk)
            assert _blocks(l, 3, 1000, 6) > 1 and 1000 % rpb, l
        # the cap of 64 slabs per image is the term that binds in both statistics passes
        for l in ("fwd_stats", "bwd_stats"):
            unr, target, max_blk = LAUNCHES[l]
            assert max_blk == 64 and min(target, 4096 // (6 * unr)) > max_blk and 1 < _blocks(l, 1, 4096, 6) <= 64
        assert any(B == 40 and HW == 16 for _, B, HW in shapes)
        # the second stage of dgamma / dbeta is reached with one slice and with several
        sl = {_slices(B * _blocks("bwd_stats", B, HW, rif_of[Cc])) for Cc, B, HW in shapes}
        assert {1, 4} <= sl
    for Cc in MODEL_WIDTHS:
        assert ("bf16", Cc) in FORMS, Cc
    assert {_slots(n) for n in range(1, 769)} == {1, 2, 3}


def test_workspace_promises():
    """Host only: the slabs of every grid the rule produces fit what pdmk.h promises for `ws` and `part_ws`."""
    from pdm import _pdmk as k
    for (dn, Cc), ((tpr, rif, slots), (G, gs), _) in FORMS.items():
        for B in (1, 2, 8, 16, 32, 64):
            for HW in (1, 64, 256, 1024, 4096, 16384):
                nblk, n = k._dims(k._lib.pdmk_groupnorm_bwd_partial_dims, B, HW, Cc, G, gs, k.BF16 if dn == "bf16" else k.F32)
                assert n == G * gs, (dn, Cc, n)
                assert nblk == B * _blocks("bwd_stats", B, HW, rif), (dn, Cc, B, HW, nblk)
                assert nblk * 2 * n * 4 <= k._lib.pdmk_groupnorm_bwd_part_workspace_bytes(G, gs), (dn, Cc, B, HW, nblk)
                for l in ("fwd_stats", "bwd_stats"):               # [B][blocks][G][2] floats in `ws`
                    nb = _blocks(l, B, HW, rif)
                    assert 1 <= nb <= 64 and B * nb * G * 2 * 4 <= k._lib.pdmk_groupnorm_workspace_bytes(B, G), (dn, Cc, B, HW, l)
    a, b = k.i32(0), k.i32(0)
    assert k._lib.pdmk_groupnorm_bwd_partial_dims(2, 64, 324, 32, 10, k.BF16, C.byref(a), C.byref(b)) == -1   # C % 8


PAD, ROWS_AFTER, SENT = 8, 3, 7.0


def _strided(B, HW, Cc, dev, dt, fill=None):
    """[B, HW, Cc] view with row stride Cc + 16 that starts 8 columns into its buffer; ROWS_AFTER rows follow it."""
    M = B * HW
    if fill is None:
        buf = torch.randn(M + ROWS_AFTER, Cc + 2 * PAD, device=dev).to(dt)
    else:
        buf = torch.full((M + ROWS_AFTER, Cc + 2 * PAD), fill, device=dev, dtype=dt)
    return buf, buf[:M, PAD:PAD + Cc].unflatten(0, (B, HW))


def _sentinels_intact(buf, M, Cc, what):
    assert bool((buf[:, :PAD] == SENT).all()) and bool((buf[:, PAD + Cc:] == SENT).all()), f"{what}: columns beside the view written"
    assert bool((buf[M:] == SENT).all()), f"{what}: rows after the last written"


def _loguniform(shape, dev, lo=0.25, hi=4.0):
    return torch.exp(torch.empty(shape, device=dev, dtype=torch.float64).uniform_(math.log(lo), math.log(hi)))


def _block_check(check, dn, case, got, ref, tol, dims):
    """max |got - ref| <= tol * max |ref| over every block (`dims` are the dimensions inside a block); prints before it asserts"""
    err = (got.double() - ref).abs().amax(dims)
    scale = ref.abs().amax(dims)
    rel = float((err / scale.clamp_min(1e-300)).max())
    print(f"GN_PARITY {check} {dn} {case} rel={rel:.3e} tol={tol:.1e}")
    assert bool(torch.isfinite(got.float()).all()), f"{check} {dn} {case}: non-finite values"
    assert bool((err <= tol * scale).all()), f"{check} {dn} {case}: worst block {rel:.3e} of its scale (tol {tol})"


def _reference(x, gamma, beta, dy, G, gs, silu):
    """fp64: (y, mean, var, rstd, dx, dgamma, dbeta), the tensors in [B, HW, G, gs] / [B, G] / [G, gs]"""
    B, HW = x.shape[:2]
    cr = G * gs
    xd = x.double()[..., :cr].reshape(B, HW, G, gs).clone().requires_grad_(True)
    gd = gamma.double().view(G, gs).clone().requires_grad_(True)
    bd = beta.double().view(G, gs).clone().requires_grad_(True)
    mean = xd.mean((1, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = (var + EPS) ** -0.5
    z = (xd - mean) * rstd * gd + bd
    y = z * torch.sigmoid(z) if silu else z
    gx, gg, gb = torch.autograd.grad(y, [xd, gd, bd], dy.double()[..., :cr].reshape(B, HW, G, gs))
    return y.detach(), mean.detach().view(B, G), var.detach().view(B, G), rstd.detach().view(B, G), gx, gg, gb


def _check_stats(dn, case, stats, mean, var, rstd):
    tol = TOL["f32"]
    got_m, got_r = stats[..., 0].double(), stats[..., 1].double()
    assert bool(torch.isfinite(stats).all()), f"{case}: statistics not written"
    rel_r = float(((got_r - rstd).abs() / rstd).max())
    rel_m = float(((got_m - mean).abs() / (mean.abs() + var.sqrt())).max())
    print(f"GN_PARITY rstd {dn} {case} rel={rel_r:.3e} tol={tol:.1e}")
    print(f"GN_PARITY mean {dn} {case} rel={rel_m:.3e} tol={tol:.1e}")
    assert rel_r <= tol, f"{case}: rstd off by {rel_r:.3e} relative"
    assert rel_m <= tol, f"{case}: mean off by {rel_m:.3e} of |mean| + std"


def _guarded(n, dev, dtype):
    """exactly n elements with 32 sentinel elements on either side"""
    buf = torch.full((n + 64,), -123.0, device=dev, dtype=dtype)
    return buf, buf[32:32 + n]


def _guards_intact(buf, n, what):
    assert bool((buf[:32] == -123.0).all()) and bool((buf[32 + n:] == -123.0).all()), what


def _unaligned(t):
    """the same fp32 values in a slice that starts one float into its buffer"""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=torch.float32)
    u = buf[1:1 + t.numel()]
    u.copy_(t)
    assert t.data_ptr() % 16 == 0 and u.data_ptr() % 16 == 4
    return u


@pytest.mark.gpu
@pytest.mark.parametrize("dn,Cc,B,HW", _cases())
def test_groupnorm_forms(dev, dn, Cc, B, HW):
    for silu in (False, True):
        _run_case(dev, dn, Cc, B, HW, silu)


def _run_case(dev, dn, Cc, B, HW, silu):
    from pdm import _pdmk as k
    (tpr, rif, slots), (G, gs), _ = FORMS[(dn, Cc)]
    torch.manual_seed(100000 * silu + 10 * Cc + B + HW)
    dt = DT[dn]
    M, cr, ld = B * HW, G * gs, Cc + 2 * PAD
    case = f"{B}x{HW}x{Cc} G{G}x{gs} silu={int(silu)}"
    # every (image, group) has its own mean and scale (module docstring); padding channels stay plain randn
    noise = torch.randn(B, HW, G, gs, device=dev, dtype=torch.float64)
    noise = noise - noise.mean((1, 3), keepdim=True)
    noise = noise / noise.pow(2).mean((1, 3), keepdim=True).sqrt()
    sigma, sdy = _loguniform((B, 1, G, 1), dev), _loguniform((B, 1, G, 1), dev)
    u = torch.empty(B, 1, G, 1, device=dev, dtype=torch.float64).uniform_(-3, 3)
    xbuf, x = _strided(B, HW, Cc, dev, dt)
    x[..., :cr] = (sigma * (noise + u)).reshape(B, HW, cr).to(dt)
    dybuf, dy = _strided(B, HW, Cc, dev, dt)
    dy[..., :cr] = (sdy * torch.randn(B, HW, G, gs, device=dev, dtype=torch.float64)).reshape(B, HW, cr).to(dt)
    gamma, beta = torch.randn(cr, device=dev) * 0.5 + 1, torch.randn(cr, device=dev) * 0.5
    ref_y, mean, var, rstd, ref_dx, ref_dg, ref_db = _reference(x, gamma, beta, dy, G, gs, silu)
    need = k._lib.pdmk_groupnorm_workspace_bytes(B, G) // 8
    wsbuf, ws = _guarded(need, dev, torch.float64)
    gamma_u, beta_u = _unaligned(gamma), _unaligned(beta)

    # ---- forward: twice with aligned gamma / beta, once with unaligned ones
    def fwd(gm, bt):
        ybuf, y = _strided(B, HW, Cc, dev, dt, fill=SENT)
        stats = torch.full((B, G, 2), float("nan"), device=dev)
        k.groupnorm_fwd(x, y, gm, bt, stats, ws, B, HW, Cc, ld, ld, G, gs, EPS, silu)
        return ybuf, y, stats

    ybuf, y, stats = fwd(gamma, beta)
    print(f"GN_DIGEST {dn} {case} ybuf {digest(ybuf)}")
    print(f"GN_DIGEST {dn} {case} stats {digest(stats)}")
    _check_stats(dn, case, stats, mean, var, rstd)
    _block_check("y", dn, case, y[..., :cr].reshape(B, HW, G, gs), ref_y, TOL[dn], (1, 3))
    assert bool((y[..., cr:] == 0).all()), case + ": padding channels of y"
    _sentinels_intact(ybuf, M, Cc, case + " y")
    for gm, bt, what in ((gamma, beta, "between two runs"), (gamma_u, beta_u, "with unaligned gamma / beta")):
        ybuf2, y2, stats2 = fwd(gm, bt)
        assert torch.equal(y, y2) and torch.equal(stats, stats2), f"{case}: y / stats differ {what}"
        _sentinels_intact(ybuf2, M, Cc, case + " y " + what)

    # ---- backward, from statistics built here
    stats_ref = torch.stack([mean, rstd], -1).float().contiguous()
    dscale = (sdy / sigma).expand(B, HW, G, gs).reshape(B, HW, cr)          # the scale of dx in a block: rstd * |gamma * dy|
    base, (addbuf, add) = torch.randn(B, HW, Cc, device=dev), _strided(B, HW, Cc, dev, dt)
    base[..., :cr] *= dscale
    base = base.to(dt)
    add[..., :cr] = (add[..., :cr].double() * dscale).to(dt)
    add_rows = addbuf[:M, PAD:PAD + Cc]                  # the wrapper takes `add` as [M, C] and its row stride from stride(0)
    assert add_rows.data_ptr() == add.data_ptr() and add_rows.stride(0) == ld
    dg0 = torch.randn(cr, device=dev) * ref_dg.abs().amax(1, keepdim=True).expand(G, gs).reshape(cr).float()
    db0 = torch.randn(cr, device=dev) * ref_db.abs().amax(1, keepdim=True).expand(G, gs).reshape(cr).float()
    nblk, n = k._dims(k._lib.pdmk_groupnorm_bwd_partial_dims, B, HW, Cc, G, gs, k.dt(x))
    assert n == cr and nblk == B * _blocks("bwd_stats", B, HW, rif)

    def bwd(acc, with_add, gm=gamma, bt=beta):
        dxbuf, dx = _strided(B, HW, Cc, dev, dt, fill=SENT)
        dx.copy_(base if acc else torch.full_like(base, float("nan")))     # without accumulate dx is overwritten, never read
        dg, db = dg0.clone(), db0.clone()
        k.groupnorm_bwd(x, dy, dx, gm, bt, stats_ref, dg, db, ws, B, HW, Cc, ld, ld, ld, G, gs, silu, acc,
                        add=add_rows if with_add else None)
        return dxbuf, dx, dg, db

    direct = None
    for acc in (False, True):
        for with_add in (False, True):
            what = f"{case} acc={int(acc)} add={int(with_add)}"
            dxbuf, dx, dg, db = bwd(acc, with_add)
            print(f"GN_DIGEST {dn} {what} dxbuf {digest(dxbuf)}")
            if _slices(nblk) == 1:
                print(f"GN_DIGEST {dn} {what} dgamma {digest(dg)}")
                print(f"GN_DIGEST {dn} {what} dbeta {digest(db)}")
            extra = (base.double() if acc else 0.0) + (add.double() if with_add else 0.0)
            ref = ref_dx + (extra[..., :cr].reshape(B, HW, G, gs) if acc or with_add else 0.0)
            _block_check("dx", dn, what, dx[..., :cr].reshape(B, HW, G, gs), ref, 2 * TOL[dn], (1, 3))
            # the parameter gradients accumulate into non-zero values; the error is measured against the gradient alone
            for name, got, start, rg in (("dgamma", dg, dg0, ref_dg), ("dbeta", db, db0, ref_db)):
                err = (got.double().view(G, gs) - start.double().view(G, gs) - rg).abs().amax(1)
                scale = rg.abs().amax(1)
                rel = float((err / scale.clamp_min(1e-300)).max())
                print(f"GN_PARITY {name} {dn} {what} rel={rel:.3e} tol={2 * TOL[dn]:.1e}")
                assert bool((err <= 2 * TOL[dn] * scale).all()), f"{name} {dn} {what}: {rel:.3e}"
            pad_ref = torch.zeros(B, HW, Cc - cr, device=dev)
            if acc:
                pad_ref = pad_ref + base[..., cr:].float()
            if with_add:
                pad_ref = pad_ref + add[..., cr:].float()
            assert torch.equal(dx[..., cr:], pad_ref.to(dt)), what + ": padding channels of dx"
            _sentinels_intact(dxbuf, M, Cc, what + " dx")
            _, dx2, dg2, db2 = bwd(acc, with_add)
            assert torch.equal(dx, dx2), what + ": dx differs between two runs"
            if _slices(nblk) == 1:
                assert torch.equal(dg, dg2) and torch.equal(db, db2), what + ": dgamma / dbeta differ between two runs"
            if acc and with_add:
                direct = (dx, dg, db)
    dxbuf, dx, dg, db = bwd(True, True, gamma_u, beta_u)
    assert torch.equal(dx, direct[0]), case + ": dx differs with unaligned gamma / beta"
    _sentinels_intact(dxbuf, M, Cc, case + " dx, unaligned gamma / beta")
    if _slices(nblk) == 1:
        assert torch.equal(dg, direct[1]) and torch.equal(db, direct[2]), case + ": dgamma / dbeta differ with unaligned gamma / beta"

    # ---- the slabs fit exactly what pdmk_groupnorm_bwd_partial_dims says; one float short is refused
    pbuf, part = _guarded(nblk * 2 * n, dev, torch.float32)
    dxbuf, dx = _strided(B, HW, Cc, dev, dt, fill=SENT)
    dx.copy_(base)
    dg, db = dg0.clone(), db0.clone()

    def raw(elems):
        return k._lib.pdmk_groupnorm_bwd(k._p(x), k._p(dy), k._p(dx), k._p(gamma), k._p(beta), k._p(stats_ref), k._p(dg), k._p(db),
                                         k._p(ws), k._p(part), elems, B, HW, Cc, ld, ld, ld, G, gs, int(silu), 1, k._p(add), ld,
                                         k.dt(x), k._st())

    assert raw(part.numel() - 1) == -1
    torch.cuda.synchronize()
    assert torch.equal(dx, base) and torch.equal(dg, dg0), case + ": a refused call wrote its outputs"
    assert raw(part.numel()) == 0
    torch.cuda.synchronize()
    _guards_intact(pbuf, part.numel(), case + ": partial slabs overrun")
    _guards_intact(wsbuf, need, case + ": statistics slabs overrun")
    assert torch.equal(dx, direct[0]), case + ": dx differs with an exact-size part_ws"
    for a, b, s in ((dg, direct[1], dg0), (db, direct[2], db0)):
        close(a - s, b - s, 1e-4, case + " exact-size part_ws")


def _exact_inputs(dev, dt, B, HW, Cc, G, gs):
    """x = m[b, g] + d, integers of magnitude <= 65 with |m| >= 32 in every other group: every fp32 sum of x and x^2 is exact"""
    m = torch.randint(-64, 65, (B, 1, G, 1), device=dev)
    big = torch.randint(32, 65, (B, 1, G, 1), device=dev) * (2 * torch.randint(0, 2, (B, 1, G, 1), device=dev) - 1)
    sel = (torch.arange(G, device=dev).view(1, 1, G, 1) + torch.arange(B, device=dev).view(B, 1, 1, 1)) % 2 == 0
    m = torch.where(sel, big, m)
    d = torch.randint(-1, 2, (B, HW, G, gs), device=dev)
    xg = (m + d).reshape(B, HW, G * gs)
    assert int(xg.abs().max()) <= 65 and int((m.abs() >= 32).sum()) * 2 >= B * G
    x = torch.zeros(B, HW, Cc, device=dev, dtype=dt)
    x[..., :G * gs] = xg.to(dt)
    assert torch.equal(x[..., :G * gs].long(), xg)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("dn", ["bf16", "f32"])
def test_groupnorm_cancellation_with_exact_sums(dev, dn):
    """|mean| up to 80 x std, with inputs whose fp32 sums are exact in any order: what is left between the kernel's statistics and
    fp64 is the double -> float rounding of the mean (1 ulp) and, for rstd, the rounding of var + eps to float (<= 0.25 ulp of
    rstd), the 1-ulp v_rsq and one Newton step, which squares that error and adds three roundings of its own - about 2 ulp,
    held to 4.  The same inputs through an fp32 1 / n and an fp32 mean^2 give 1.9e-4 relative, 400 x the bound."""
    from pdm import _pdmk as k
    dt = DT[dn]
    wide = (2, 48, 2560, 32, 80) if dn == "bf16" else (2, 64, 1280, 32, 40)           # slots = 2
    for B, HW, Cc, G, gs in ((2, 64, 80, 8, 10), wide):
        assert HW * gs * 4225 < 2 ** 24 and Cc == G * gs
        torch.manual_seed(Cc)
        case = f"exact {B}x{HW}x{Cc} G{G}x{gs}"
        x = _exact_inputs(dev, dt, B, HW, Cc, G, gs)
        dy = (torch.randn(B, HW, Cc, device=dev)).to(dt)
        gamma, beta = torch.randn(Cc, device=dev) * 0.5 + 1, torch.randn(Cc, device=dev) * 0.5
        ref_y, mean, var, rstd, ref_dx, ref_dg, ref_db = _reference(x, gamma, beta, dy, G, gs, True)
        assert float((mean.abs() / var.sqrt()).max()) > 30
        y = torch.full_like(x, SENT)
        stats = torch.full((B, G, 2), float("nan"), device=dev)
        ws = k.groupnorm_ws(dev, B, G)
        k.groupnorm_fwd(x, y, gamma, beta, stats, ws, B, HW, Cc, Cc, Cc, G, gs, EPS, True)
        m32 = mean.float()
        ulp = torch.nextafter(m32.abs(), torch.full_like(m32, float("inf"))) - m32.abs()
        mean_ulps = float(((stats[..., 0] - m32).abs() / ulp).max())
        rstd_ulps = float(((stats[..., 1].double() - rstd).abs() / rstd).max()) * 2.0 ** 23
        print(f"GN_PARITY exact_mean_ulp {dn} {case} rel={mean_ulps:.3e} tol={1.0:.1e}")
        print(f"GN_PARITY exact_rstd_ulp {dn} {case} rel={rstd_ulps:.3e} tol={4.0:.1e}")
        assert mean_ulps <= 1.0, f"{case}: mean {mean_ulps} ulp from float32(fp64 mean)"
        assert rstd_ulps <= 4.0, f"{case}: rstd {rstd_ulps:.2f} x 2^-23 relative from fp64"
        _block_check("exact_y", dn, case, y.reshape(B, HW, G, gs), ref_y, TOL[dn], (1, 3))
        stats_ref = torch.stack([mean, rstd], -1).float().contiguous()
        dx = torch.full_like(x, SENT)
        dg, db = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
        k.groupnorm_bwd(x, dy, dx, gamma, beta, stats_ref, dg, db, ws, B, HW, Cc, Cc, Cc, Cc, G, gs, True, False)
        _block_check("exact_dx", dn, case, dx.reshape(B, HW, G, gs), ref_dx, 2 * TOL[dn], (1, 3))
        _block_check("exact_dgamma", dn, case, dg.view(G, gs), ref_dg, 2 * TOL[dn], (1,))
        _block_check("exact_dbeta", dn, case, db.view(G, gs), ref_db, 2 * TOL[dn], (1,))


@pytest.mark.gpu
@pytest.mark.parametrize("dn", ["bf16", "f32"])
def test_groupnorm_rejections(dev, dn):
    """Every -1 of gn_fwd / gn_bwd, one argument off a call that is accepted, on the raw entry points.  (On the GPU and with device
    buffers that would hold every one of these shapes: a rejection that went missing would launch, and must then not run on
    pointers that are not device memory.)"""
    from pdm import _pdmk as k
    dt, v = DT[dn], V[dn]
    cap = 3 * NT * v
    rows, wid = 8, cap + 2 * v
    x, dy, add = (torch.randn(rows * wid + 8, device=dev).to(dt) for _ in range(3))
    y, dx = torch.zeros(rows * wid + 8, device=dev, dtype=dt), torch.zeros(rows * wid + 8, device=dev, dtype=dt)
    gamma, beta = torch.ones(wid, device=dev), torch.zeros(wid, device=dev)
    stats = torch.zeros(2, 65, 2, device=dev)
    stats[..., 1] = 1.0
    ws = k.groupnorm_ws(dev, 2, 65)
    part = torch.zeros(1 << 20, device=dev)
    dg, db = torch.zeros(wid, device=dev), torch.zeros(wid, device=dev)
    ok = dict(B=2, HW=4, C=128, ldx=128, G=8, gs=8, elems=part.numel(), add=None)

    def fwd(B, HW, C, ldx, G, gs, elems, add):
        return k._lib.pdmk_groupnorm_fwd(k._p(x), k._p(y), k._p(gamma), k._p(beta), k._p(stats), k._p(ws), B, HW, C, ldx, wid, G, gs,
                                         EPS, 1, k.dt(x), k._st())

    def bwd(B, HW, C, ldx, G, gs, elems, add):       # every other leading dimension is `wid`: only the argument named is off
        return k._lib.pdmk_groupnorm_bwd(k._p(x), k._p(dy), k._p(dx), k._p(gamma), k._p(beta), k._p(stats), k._p(dg), k._p(db),
                                         k._p(ws), k._p(part), elems, B, HW, C, ldx, wid, wid, G, gs, 1, 0, add,
                                         0 if add is None else wid, k.dt(x), k._st())

    nblk, n = k._dims(k._lib.pdmk_groupnorm_bwd_partial_dims, 2, 4, 128, 8, 8, k.dt(x))
    both = {
        "G = 65": dict(G=65, gs=1),
        "G * gs > C": dict(gs=17),
        "C not a multiple of the vector width": dict(C=128 - v // 2, ldx=256),
        "ldx not a multiple of the vector width": dict(ldx=128 + v // 2),
        "C one vector past the capacity": dict(C=cap + v, ldx=cap + v),
    }
    assert cap + v == (6152 if dn == "bf16" else 3076)
    for f in (fwd, bwd):
        assert f(**ok) == 0
        assert f(**{**ok, "C": cap, "ldx": cap}) == 0, "the capacity itself is accepted"
        assert f(**{**ok, "G": 64, "gs": 2}) == 0
        for why, ch in both.items():
            assert f(**{**ok, **ch}) == -1, why
    assert bwd(**{**ok, "elems": nblk * 2 * n}) == 0
    assert bwd(**{**ok, "elems": nblk * 2 * n - 1}) == -1, "part_ws one float short"
    assert add.data_ptr() % 16 == 0
    assert bwd(**{**ok, "add": add.data_ptr()}) == 0
    assert bwd(**{**ok, "add": add.data_ptr() + add.element_size()}) == -1, "add not 16-byte aligned"
    torch.cuda.synchronize()
    # the wrapper reads the row stride of `add` from stride(0): an [B, HW, C] view (stride(0) = HW rows) is refused before any launch
    with pytest.raises(k.PdmkError):
        k.groupnorm_bwd(x, dy, dx, gamma, beta, stats, dg, db, ws, 2, 4, 128, wid, wid, wid, 8, 8, True, False,
                        add=add[:8 * wid].view(2, 4, wid)[..., :128])
