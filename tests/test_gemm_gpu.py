"""GEMM kernels against fp64 (-m gpu): every dispatch form, epilogue branch and stride, each under a candidate the test forces and
then ASSERTS (k.last_candidate(), k.last_form()) against an expectation written here from the documented rules:
  - PDMK_RING_CFG / PDMK_WGRAD_CFG = 0 is candidate 0: igemm_kernel KCH 8 (form 1) up to 512 workgroups, KCH 4 (form 2) above;
    bf16 forward problems go to igemm_dma_kernel instead from 384 128x128 blocks on, or always under PDMK_GEMM_DMA=2 (conv modes
    0..3 only), with 128-row tiles (form 3) below 320 256-row blocks and 256-row tiles (form 4) from there on;
  - the forward ring rows (candidates 1..12, 17..19) serve every bf16 forward problem; the halo ids 13..16 stride-1 convs with
    packed weights on images their placement rules accept; the weight-gradient rings 1..5 every bf16 weight gradient with fp32
    output, the halo weight gradients 6, 7 stride-1 convs on images that fill 128-pixel blocks, with at most one split per block;
    whatever a forced candidate does not serve falls back to candidate 0.
Inputs, the fp64 reference and the derived elementwise bound are tests/gemm_fixtures.py's: operands are slices of wider NaN-filled
buffers (lda, ldb, conv_ld, ldr, ldrv, ldc above the used extent, rowvec at a column offset), C sits between sentinels.  Every
comparison asserts max |got - ref| / bound <= 1, finite values and bit-unchanged sentinels, and prints a GEMM_PARITY line
(profiles/gemm_parity.txt is a collected run).  There is no second, looser tolerance."""
import os
import zlib

import pytest
import torch

import gemm_fixtures as gf

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
VARS = ("PDMK_RING_CFG", "PDMK_WGRAD_CFG", "PDMK_GEMM_DMA")
RING_FWD = list(range(1, 13)) + [17, 18, 19]
RING_BM = {256: 1, 128: 3, 64: 5}          # one forward ring row of each tile height (gemm_ring.hip kRing: row = id - 1)
HALO = [13, 14, 15, 16]
CONV_HW = {0: ((6, 10), (7, 9)), 1: ((7, 9),), 2: ((6, 10), (7, 9)), 3: ((6, 10), (7, 9)), 4: ((6, 10),)}


@pytest.fixture
def force():
    """force(ring=, wgrad=, dma=): set PDMK_RING_CFG / PDMK_WGRAD_CFG / PDMK_GEMM_DMA (None = unset); restored afterwards."""
    saved = {v: os.environ.get(v) for v in VARS}
    for v in VARS:
        os.environ.pop(v, None)

    def setter(ring=None, wgrad=None, dma=None):
        for var, val in zip(VARS, (ring, wgrad, dma)):
            if val is None:
                os.environ.pop(var, None)
            else:
                os.environ[var] = str(val)
    yield setter
    for v in VARS:
        os.environ.pop(v, None)
        if saved[v] is not None:
            os.environ[v] = saved[v]


_PROBLEMS = {}


def problem(dev, keep=True, **kw):
    """Problems (and their fp64 references) are built once and shared by the candidates that run them."""
    key = tuple(sorted((k, str(v)) for k, v in kw.items()))
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    # the seed depends on the operands only: problems that differ in the epilogue alone share A and B (slabs and their finish)
    seed = zlib.crc32(repr([str(kw.get(a)) for a in ("kind", "dtype", "M", "N", "K", "conv", "tight_b")]).encode()) % 100000
    p = gf.make_problem(dev=dev, seed=seed, **kw)
    if keep:
        _PROBLEMS[key] = p
    return p


def launch(k, p, cv, sv):
    c = p.conv
    k.gemm(p.A, p.B, cv, p.M, p.N, p.K, p.lda, p.ldb, p.ldc, bias=p.bias, rowvec=p.rv, rows_per_b=p.rows_per_b, R=p.R,
           ldr=p.ldr, a_mode=p.a_mode, b_mode=p.b_mode,
           conv=None if c is None else (c.b, c.hi, c.wi, c.ci, c.ho, c.wo, c.mode, c.ld),
           out_f32=p.out_f32 and p.dtype == BF, accumulate=p.accumulate, splitk=p.splitk, alpha=p.alpha, colsum_out=sv,
           ldrv=p.ldrv)


def run(k, p, expect, label):
    """One pdmk_gemm on fresh output buffers: the kernel that ran is asserted, then the result is checked."""
    cb, cv, sb, sv = gf.fresh_outputs(p)
    launch(k, p, cv, sv)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a device fault: nothing more may run on this GPU
        pytest.exit(f"{label}: device error after pdmk_gemm: {e}", returncode=3)
    ran = (k.last_candidate(), k.last_form())
    name = f"{label} {p.kind} {p.M}x{p.N}x{p.K} sk{p.splitk} {'bf16' if p.dtype == BF else 'f32'} cand={ran[0]} form={ran[1]}"
    r = gf.check(p, cb, cv, sb, sv, label=name)
    assert ran == expect, f"{label}: candidate / form {ran} ran, expected {expect}"
    return r, cb


def run_slab_finish(k, p, pf, expect, label):
    """Slab split-K (p: accumulate = 2) followed by pdmk_splitk_finish with pf's epilogue operands into pf's C."""
    _, cb = run(k, p, expect, label + " slabs")
    fb, fv, _, _ = gf.fresh_outputs(pf)
    k.splitk_finish(cb, fv, pf.M, pf.N, pf.ldc, pf.splitk, bias=pf.bias, rowvec=pf.rv, R=pf.R, ldr=pf.ldr,
                    rows_per_b=pf.rows_per_b, ldrv=pf.ldrv, accumulate=pf.prev is not None)
    torch.cuda.synchronize()
    gf.check(pf, fb, fv, label=f"{label} finish {pf.M}x{pf.N}x{pf.K} sk{pf.splitk}")


# ------------------------------------------------------------------------------------------------------------ A. epilogues
EPI = dict(bias=True, rowvec=True, residual=True, rows_per_b=100)


def epilogue_branches(dev):
    """(label, problem, finish problem or None) of every epilogue branch, on N = 200 (vec8) and N = 196 (N % 8: scalar)."""
    out = []
    for N in (200, 196):
        lin = dict(kind="linear", dtype=BF, M=300, N=N)
        out += [
            (f"epilogue N{N}", problem(dev, K=160, **lin, **EPI), None),
            (f"accumulate alpha N{N}", problem(dev, K=160, accumulate=1, alpha=0.5, bias=True, **lin), None),
            (f"out_f32 N{N}", problem(dev, K=32, out_f32=True, bias=True, **lin), None),
            (f"out_f32 accumulate N{N}", problem(dev, K=32, out_f32=True, accumulate=1, alpha=0.5, **lin), None),
            (f"atomic split N{N}", problem(dev, K=608, out_f32=True, splitk=3, **lin, **EPI), None),
            # 4 splits over K = 160: three K-steps of 64 (five of 32) - the last split is empty and still owes its zero slab
            (f"slab split N{N}", problem(dev, K=160, out_f32=True, splitk=4, accumulate=2, **lin),
             problem(dev, K=160, splitk=4, **lin, **EPI)),
            (f"scalar strides N{N}", problem(dev, K=160, scalar=True, **lin, **EPI), None),
            (f"scalar strides out_f32 accumulate N{N}", problem(dev, K=160, scalar=True, out_f32=True, accumulate=1, **lin, **EPI),
             None),
        ]
    return out


@pytest.mark.parametrize("cand", [0] + RING_FWD)
def test_epilogue_matrix(dev, force, cand):
    from pdm import _pdmk as k
    force(ring=cand)
    expect = (cand, 0) if cand else (0, 1)
    for label, p, pf in epilogue_branches(dev):
        if pf is None:
            run(k, p, expect, f"A cand{cand} {label}")
        else:
            run_slab_finish(k, p, pf, expect, f"A cand{cand} {label}")


# ------------------------------------------------------------------------------------------------------------ B. conv gathers
def conv_problems(dev, mode, **kw):
    return [problem(dev, kind="conv", dtype=BF, N=40, conv=(2, h, w, 32, mode), bias=True, rowvec=True, **kw)
            for h, w in CONV_HW[mode]]


# (igemm_dma_kernel has no mode-4 gather: pdmk_gemm_dma_launch refuses it)
@pytest.mark.parametrize("mode,target", [(m, t) for m in (0, 1, 2, 3, 4) for t in ("cand0", "dma", "ring64", "ring128", "ring256")
                                         if not (m == 4 and t == "dma")])
def test_conv_gathers(dev, force, mode, target):
    """Strided (conv_ld 48 > ci 32) rectangular images, 32 -> 40 channels, bias + sliced rowvec."""
    from pdm import _pdmk as k
    if target == "dma":
        force(ring=0, dma=2)
        expect = (0, 3)
    elif target == "cand0":
        force(ring=0)
        expect = (0, 1)
    else:
        cand = RING_BM[int(target[4:])]
        force(ring=cand)
        expect = (cand, 0)
    for p in conv_problems(dev, mode):
        run(k, p, expect, f"B {target} mode{mode} {p.conv.hi}x{p.conv.wi}")


@pytest.mark.parametrize("cand", HALO)
def test_conv_halo_ids(dev, force, cand):
    """Halo ids: stride 1, packed weights (ldb = 9 ci); three 8 x 16 images = 128-pixel tiles (256-row tiles hold two, the
    last tile one) and two 16 x 16 images; the strided modes fall back to candidate 0."""
    from pdm import _pdmk as k
    force(ring=cand)
    for Bn, h, w in ((3, 8, 16), (2, 16, 16)):
        p = problem(dev, kind="conv", dtype=BF, N=40, conv=(Bn, h, w, 32, 0), bias=True, rowvec=True, residual=True, tight_b=True)
        run(k, p, (cand, 0), f"B halo{cand} mode0 {h}x{w}")
    p = problem(dev, kind="conv", dtype=BF, N=40, conv=(2, 7, 9, 32, 1), bias=True, rowvec=True, tight_b=True)
    run(k, p, (0, 1), f"B halo{cand} mode1 7x9 (not served)")


# ------------------------------------------------------------------------------------------------------------ C. candidate-0 forms
def big_conv(mode):
    """Image sizes with 48 x 40 output pixels: 2 images = 3840 rows = 30 tiles of 128."""
    return {0: (48, 40), 1: (95, 80), 2: (24, 20), 3: (24, 20), 4: (96, 80)}[mode]


@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_kch4_linear(dev, force, dn):
    """igemm_kernel KCH 4 takes grids above 512 workgroups: 23 x 24 tiles of a wide one-K-step GEMM (stores in dtype), and
    6 tiles x 86 splits (fp32 atomics, epilogue operands added by the first split only)."""
    from pdm import _pdmk as k
    force(ring=0, dma=0)                 # bf16: without PDMK_GEMM_DMA=0 these grids go to igemm_dma_kernel (test_dma_forms)
    dt = F32 if dn == "f32" else BF
    p = problem(dev, keep=False, kind="linear", dtype=dt, M=2900, N=2990, K=32, bias=True, rowvec=True, residual=True, rows_per_b=1000)
    run(k, p, (0, 2), f"C kch4 {dn} wide")
    p = problem(dev, keep=False, kind="linear", dtype=dt, M=300, N=196, K=2752, out_f32=True, splitk=86, **EPI)
    run(k, p, (0, 2), f"C kch4 {dn} 86 splits")


@pytest.mark.parametrize("dn", ["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_kch4_conv(dev, force, dn, mode):
    from pdm import _pdmk as k
    force(ring=0, dma=0)
    dt = F32 if dn == "f32" else BF
    h, w = big_conv(mode)
    p = problem(dev, keep=False, kind="conv", dtype=dt, N=264, conv=(2, h, w, 32, mode), out_f32=True, splitk=9, bias=True,
                rowvec=True, residual=True)
    assert (p.M + 127) // 128 * 3 * 9 > 512
    run(k, p, (0, 2), f"C kch4 {dn} conv mode{mode}")


@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_kch4_weight_gradients(dev, force, dn):
    from pdm import _pdmk as k
    force(wgrad=0)
    dt = F32 if dn == "f32" else BF
    p = problem(dev, keep=False, kind="wgrad", dtype=dt, M=640, N=640, K=764, out_f32=True, splitk=24, colsum=True)   # 25 tiles x 24
    run(k, p, (0, 2), f"C kch4 {dn} wgrad linear")
    for mode, (h, w) in ((0, (32, 32)), (1, (64, 64)), (2, (16, 16))):
        p = problem(dev, keep=False, kind="wgrad_conv", dtype=dt, M=256, conv=(2, h, w, 64, mode), out_f32=True, splitk=64,
                    colsum=True)                                                                                       # 10 tiles x 64
        run(k, p, (0, 2), f"C kch4 {dn} wgrad conv mode{mode}")


def dma_cases(dev, big):
    """(label, problem): linear and conv modes 0..3 with bias, rowvec and residual, unsplit (bf16 stores) and split (atomics)."""
    out = []
    if big:         # 320 or more 256-row blocks
        out.append(("linear wide", problem(dev, keep=False, kind="linear", dtype=BF, M=2900, N=3500, K=32, bias=True, rowvec=True,
                                           residual=True, rows_per_b=1000)))                     # 12 x 28 = 336 blocks
        out.append(("linear 27 splits", problem(dev, keep=False, kind="linear", dtype=BF, M=1300, N=200, K=864, out_f32=True,
                                                splitk=27, bias=True, rowvec=True, residual=True, rows_per_b=500)))   # 6 x 2 x 27 = 324
        for mode in (0, 1, 2, 3):
            h, w = big_conv(mode)
            out.append((f"conv mode{mode} 8 splits", problem(dev, keep=False, kind="conv", dtype=BF, N=264, conv=(2, h, w, 32, mode),
                                                              out_f32=True, splitk=8, bias=True, rowvec=True, residual=True)))   # 15 x 3 x 8 = 360
    else:           # the ragged shapes, forced
        out.append(("linear", problem(dev, kind="linear", dtype=BF, M=300, N=200, K=160, **EPI)))
        out.append(("linear scalar", problem(dev, kind="linear", dtype=BF, M=300, N=196, K=160, scalar=True, **EPI)))
        out.append(("linear 3 splits", problem(dev, kind="linear", dtype=BF, M=300, N=200, K=608, out_f32=True, splitk=3, **EPI)))
        for mode in (0, 1, 2, 3):
            for h, w in CONV_HW[mode]:
                kw = dict(kind="conv", dtype=BF, N=40, conv=(2, h, w, 32, mode), bias=True, rowvec=True, residual=True)
                out.append((f"conv mode{mode} {h}x{w}", problem(dev, **kw)))
                out.append((f"conv mode{mode} {h}x{w} 3 splits", problem(dev, out_f32=True, splitk=3, **kw)))
    return out


@pytest.mark.parametrize("form", [3, 4])
def test_dma_forms(dev, force, form):
    """igemm_dma_kernel BM 128 (forced with PDMK_GEMM_DMA=2 on the ragged shapes) and BM 256 (reached by grid size)."""
    from pdm import _pdmk as k
    force(ring=0, dma=2 if form == 3 else None)
    for label, p in dma_cases(dev, big=form == 4):
        run(k, p, (0, form), f"C dma form{form} {label}")


# ------------------------------------------------------------------------------------------------------------ D. weight gradients
WG_IMAGES = {"pow2": {0: (16, 16), 1: (32, 32), 2: (8, 8)}, "div": {0: (6, 10), 1: (11, 20), 2: (3, 5)}}     # output 16x16 / 6x10
WG_LAUNCH = {"overwrite": dict(), "accumulate": dict(accumulate=1), "atomics": dict(splitk="sk"), "slabs": dict(splitk="sk", accumulate=2)}


@pytest.mark.parametrize("cand", [0, 1, 2, 3, 4, 5, 6, 7])
def test_weight_gradients(dev, force, cand):
    """dY and X are column slices of wider buffers (conv_ld 48 > ci 32); power-of-two images take the shift path of the conv
    gather, the 6 x 10 ones the division path (one K-step: the second split is empty); colsum_out rides along."""
    from pdm import _pdmk as k
    force(wgrad=cand)
    for how, extra in WG_LAUNCH.items():
        kw = {a: (3 if v == "sk" else v) for a, v in extra.items()}
        p = problem(dev, kind="wgrad", dtype=BF, M=96, N=160, K=300, out_f32=True, colsum=True, **kw)
        run(k, p, (cand, 0) if 1 <= cand <= 5 else (0, 1), f"D wcand{cand} {how} linear")
        for img, sizes in WG_IMAGES.items():
            for mode, (h, w) in sizes.items():
                kw = {a: (2 if v == "sk" else v) for a, v in extra.items()}
                p = problem(dev, kind="wgrad_conv", dtype=BF, M=64, conv=(1, h, w, 32, mode), out_f32=True, colsum=True, **kw)
                served = 1 <= cand <= 5 or (cand >= 6 and mode == 0 and img == "pow2")      # halo: stride 1, 128-pixel blocks
                run(k, p, (cand, 0) if served else (0, 1), f"D wcand{cand} {how} conv mode{mode} {img}")
