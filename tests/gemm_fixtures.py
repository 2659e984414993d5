"""Inputs, fp64 reference, derived error bound, fp32 yardstick and planted faults for the GEMM kernel tests (pure torch, CPU or
GPU; not a conftest).  tests/test_gemm_host.py proves the bound and the faults on the CPU, tests/test_gemm_gpu.py runs the kernels.

Problem.  C[M, N] = alpha * sum_k A(m, k) B(n, k) + bias[n] + rowvec[m // rows_per_b, n] + R[m, n] (+ C_prev[m, n]) as
include/pdmk.h states it, in the four operand layouts of pdmk_gemm:
    "linear"       A_ROWK x B_ROWK            A [M, K], B [N, K]
    "conv"         A_CONV x B_ROWK            A = 3x3 gather (conv_mode 0..4) of an NHWC image, B [N, 9 ci]
    "wgrad"        A_COLK x B_COLK            A = dY [K, M], B = X [K, N]              (K = pixels)
    "wgrad_conv"   A_COLK x B_COLK_CONV       A = dY [K, M], B = 3x3 gather of the image X, N = 9 ci (conv_mode 0..2)
Every operand is a slice of a WIDER buffer filled with NaN, the way the engine passes channel slices of concat buffers: lda, ldb,
conv_ld, ldr and ldrv exceed the used extent and every slice starts at a column offset (16-byte aligned, as pdmk.h demands; the
"scalar" layout uses odd ldc / ldr / ldrv and odd offsets for C, R and rowvec, which only the scalar epilogue can take).  A kernel
that reads past an extent gets NaN.  C lies inside a buffer of SENTINEL values with columns left and right of the N used ones and
rows behind the M used ones: check() demands them bit-unchanged.

Reference.  ref() evaluates the formula in fp64 on the CPU from the stored inputs (bf16 / fp32 values are exact in fp64);
convs go through F.conv2d, weight gradients through its autograd.  The same evaluation on absolute values gives S.

Bound (derived, not measured).  A sum of n fp32 terms, in ANY order, with or without fused multiply-adds, is within
(n - 1) u of the exact sum relative to the sum of absolute values, u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, 4.2 - the bound does not depend on the order, hence not on tiles, K-steps, splits or atomics).  A GEMM element adds
K products (one rounding each, or none under FMA), one partial per split and at most 8 epilogue terms and scalings (alpha, bias,
rowvec, residual, previous C, slab sums): n <= K + splitk + 8.  The factor 2 covers a matrix unit whose internal accumulation
truncates instead of rounding to nearest (error per operation up to one ulp instead of half):
    gamma = 2 (K + splitk + 8) 2^-24,     fp32 output: |got - ref| <= gamma S
    bf16 output: gamma S + 2^-8 (|ref| + gamma S)      one rounding of the fp32 value to bf16 (8 significant bits)
colsum_out (the fused bias gradient) sums K = pixels terms: the same bound with S = |previous| + sum |dY|.

Yardstick.  yardstick() is the honest fp32 torch computation with the SAME split count (partial products over contiguous K
ranges, added in fp32), rounded once to the output type.  Planted faults (FAULTS) are single defects of that computation; the
host test demands yardstick <= 1.0 of the bound and every fault > 3 of it."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

SENTINEL = 1234.0
U32 = 2.0 ** -24
UBF = 2.0 ** -8
A_ROWK, A_CONV, A_COLK = 0, 1, 2
B_ROWK, B_COLK, B_COLK_CONV = 0, 1, 2
KIND_MODES = {"linear": (A_ROWK, B_ROWK), "conv": (A_CONV, B_ROWK), "wgrad": (A_COLK, B_COLK), "wgrad_conv": (A_COLK, B_COLK_CONV)}


def conv_out_hw(mode, hi, wi):
    if mode in (1, 4):
        return (hi + 1) // 2, (wi + 1) // 2
    if mode in (2, 3):
        return 2 * hi, 2 * wi
    return hi, wi


def _slice(gen, rows, cols, ld, off, dtype, dev, scale=1.0):
    """[rows, cols] random values (rounded to dtype) inside a NaN-filled [rows, ld] buffer, starting at column `off`."""
    buf = torch.full((rows, ld), float("nan"), dtype=dtype)
    buf[:, off:off + cols] = (torch.randn(rows, cols, generator=gen) * scale).to(dtype)
    buf = buf.to(dev)
    return buf, buf[:, off:off + cols]


def make_problem(kind, dev, dtype, M=0, N=0, K=0, *, conv=None, bias=False, rowvec=False, residual=False, accumulate=0,
                 out_f32=False, alpha=1.0, splitk=1, scalar=False, rows_per_b=0, colsum=False, tight_b=False, seed=0):
    """conv = (B, Hi, Wi, ci, mode): "conv" derives M and K from it (N = output channels), "wgrad_conv" K and N (M = output
    channels).  accumulate: 0 / 1 / 2 (split-K slabs: C is a [splitk, M, N] fp32 workspace, ldc = N).  scalar: odd ldc / ldr /
    ldrv and offsets.  tight_b: ldb == K (the halo kernels take packed 3x3 weights only).  The output is bf16 / fp32 as dtype
    unless out_f32."""
    gen = torch.Generator().manual_seed(1000 + seed)
    p = SimpleNamespace(kind=kind, dtype=dtype, alpha=float(alpha), splitk=int(splitk), accumulate=int(accumulate),
                        out_f32=bool(out_f32 or dtype == torch.float32), conv=None, scalar=scalar, dev=dev)
    p.a_mode, p.b_mode = KIND_MODES[kind]
    al = 8                                       # elements per 16 bytes of bf16, 32 bytes of fp32: a legal base offset for both
    if conv is not None:
        Bn, Hi, Wi, ci, mode = conv
        Ho, Wo = conv_out_hw(mode, Hi, Wi)
        ld = ci + 16
        p.img_buf, img = _slice(gen, Bn * Hi * Wi, ci, ld, al, dtype, dev)
        p.img = img                               # [Bn * Hi * Wi, ci] view, row stride conv_ld
        p.conv = SimpleNamespace(b=Bn, hi=Hi, wi=Wi, ci=ci, ho=Ho, wo=Wo, mode=mode, ld=ld)
        px = Bn * Ho * Wo
        if kind == "conv":
            M, K = px, 9 * ci
        else:
            K, N = px, 9 * ci
        rows_per_b = rows_per_b or Ho * Wo
    p.M, p.N, p.K, p.rows_per_b = M, N, K, rows_per_b
    wscale = K ** -0.5
    if kind == "linear":
        p.lda = K + 24
        p.A_buf, p.A = _slice(gen, M, K, p.lda, al, dtype, dev)
    elif kind in ("wgrad", "wgrad_conv"):
        p.lda = M + 24
        p.A_buf, p.A = _slice(gen, K, M, p.lda, al, dtype, dev)          # dY [pixels, M]
    else:
        p.lda, p.A = 0, p.img
    if kind in ("linear", "conv"):
        p.ldb = K if tight_b else K + 16
        p.B_buf, p.B = _slice(gen, N, K, p.ldb, 0 if tight_b else al, dtype, dev, wscale)
    elif kind == "wgrad":
        p.ldb = N + 40
        p.B_buf, p.B = _slice(gen, K, N, p.ldb, al, dtype, dev)          # X [pixels, N]
    else:
        p.ldb, p.B = 0, p.img
    # epilogue operands
    odd = 1 if scalar else 0
    p.bias = p.rv = p.R = p.prev = p.colsum = None
    if bias:
        p.bias_buf, b = _slice(gen, 1, N, N + 16, al, torch.float32, dev)
        p.bias = b[0]
    p.ldrv = 0
    if rowvec:
        nb = (M + rows_per_b - 1) // rows_per_b
        p.ldrv = N + 24 + odd
        p.rv_buf, p.rv = _slice(gen, nb, N, p.ldrv, 3 if scalar else al, torch.float32, dev)
    p.ldr = 0
    if residual:
        p.ldr = N + 16 + 5 * odd
        p.R_buf, p.R = _slice(gen, M, N, p.ldr, 1 if scalar else al, dtype, dev)
    odt = torch.float32 if p.out_f32 else dtype
    p.odt = odt
    if accumulate == 2:                          # slabs: [splitk][M][N] fp32, plain stores; a sentinel tail behind the last slab
        p.ldc, p.c_off, p.guard = N, 0, 64
        p.C_buf = torch.full((splitk * M * N + p.guard,), SENTINEL, dtype=torch.float32).to(dev)
    else:
        p.ldc = N + 24 + (5 if scalar else 0)
        p.c_off, p.guard = (3 if scalar else al), 2
        cb = torch.full((M + p.guard, p.ldc), SENTINEL, dtype=odt)
        if accumulate == 1 or splitk > 1:        # atomics add into what C holds: the previous C is part of the formula
            p.prev = torch.randn(M, N, generator=gen).to(odt)
            cb[:M, p.c_off:p.c_off + N] = p.prev
            p.prev = p.prev.to(dev)
        p.C_buf = cb.to(dev)
    if colsum:
        cs = torch.full((M + 16,), SENTINEL, dtype=torch.float32)
        p.colsum_prev = torch.randn(M, generator=gen)
        cs[8:8 + M] = p.colsum_prev
        p.colsum_buf = cs.to(dev)
        p.colsum = True
    return p


def fresh_outputs(p):
    """Clones of the output buffers for one run: (C buffer, C view or the flat slab workspace, colsum buffer, colsum view)."""
    cb = p.C_buf.clone()
    cv = cb if p.accumulate == 2 else cb[:p.M, p.c_off:p.c_off + p.N]
    if p.colsum:
        sb = p.colsum_buf.clone()
        return cb, cv, sb, sb[8:8 + p.M]
    return cb, cv, None, None


# ---------------------------------------------------------------------------------------------------------------- reference
def _virtual(x, mode):
    """NCHW image -> (image the 3x3 window slides over, stride, padding) of conv_mode 0..4 (include/pdmk.h)."""
    if mode == 0:
        return x, 1, 1
    if mode == 1:
        return x, 2, 1
    if mode == 2:
        return F.interpolate(x, scale_factor=2.0, mode="nearest"), 1, 1
    if mode == 3:
        up = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], dtype=x.dtype)
        up[:, :, ::2, ::2] = x
        return up, 1, 1
    return F.pad(x, (0, 1, 0, 1)), 2, 0


def _nchw(c, t):
    return t.reshape(c.b, c.hi, c.wi, c.ci).permute(0, 3, 1, 2)


def _w4(c, Bm):        # [N, 9 ci] with k = (tap, ci) -> [N, ci, 3, 3]
    return Bm.reshape(Bm.shape[0], 3, 3, c.ci).permute(0, 3, 1, 2)


def conv_geom(b, hi, wi, ci, mode):
    ho, wo = conv_out_hw(mode, hi, wi)
    return SimpleNamespace(b=b, hi=hi, wi=wi, ci=ci, ho=ho, wo=wo, mode=mode)


def product64(kind, A, B, c=None):
    """sum_k A(m, k) B(n, k) in fp64 from CPU fp64 operand values laid out as pdmk_gemm takes them (module docstring); c = the
    conv geometry (conv_geom) of the two conv kinds, whose image is [pixels, ci]."""
    if kind == "linear":
        return A @ B.t()
    if kind == "wgrad":
        return A.t() @ B
    xv, stride, pad = _virtual(_nchw(c, A if kind == "conv" else B), c.mode)
    if kind == "conv":
        y = F.conv2d(xv, _w4(c, B), stride=stride, padding=pad)
        return y.permute(0, 2, 3, 1).reshape(-1, B.shape[0])
    M = A.shape[1]
    w = torch.zeros(M, c.ci, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xv, w, stride=stride, padding=pad)
    dy = A.reshape(c.b, c.ho, c.wo, M).permute(0, 3, 1, 2)
    (gw,) = torch.autograd.grad(y, w, dy)
    return gw.permute(0, 2, 3, 1).reshape(M, 9 * c.ci)


def _d(t):
    return t.detach().cpu().double()


def formula_bound(prod, aprod, K, splitk, odt, alpha=1.0, addends=()):
    """(ref, bound) of alpha * prod + sum(addends) stored as odt, from the fp64 product and the product of absolute values."""
    ref, S = alpha * prod, abs(alpha) * aprod
    for t in addends:
        ref = ref + _d(t)
        S = S + _d(t).abs()
    bound = 2.0 * (K + splitk + 8) * U32 * S
    if odt == torch.bfloat16:
        bound = bound + UBF * (ref.abs() + bound)
    return ref, bound


def assert_within_bound(got, kind, A, B, K, *, c=None, splitk=1, alpha=1.0, addends=(), what=""):
    """One-off comparison of a kernel output (any strided view) with fp64 of the documented formula, through the derived bound."""
    A64, B64 = _d(A), _d(B)
    ref, bound = formula_bound(product64(kind, A64, B64, c), product64(kind, A64.abs(), B64.abs(), c), K, splitk, got.dtype,
                               alpha, addends)
    r = ratio(got, ref, bound)
    print(f"GEMM_PARITY {what} err/bound={r:.3f}")
    assert r <= 1.0, f"{what}: error / bound = {r:.3g} > 1"


def reference(p):
    """(ref, bound) fp64 CPU tensors [M, N]; with colsum also p.cs_ref / p.cs_bound [M].  Cached on the problem."""
    if getattr(p, "_ref", None) is not None:
        return p._ref
    A, B = _d(p.A), _d(p.B)
    rows = torch.arange(p.M)
    addends = [t for t in (p.bias, _d(p.rv)[rows // p.rows_per_b] if p.rv is not None else None, p.R, p.prev) if t is not None]
    p._ref = formula_bound(product64(p.kind, A, B, p.conv), product64(p.kind, A.abs(), B.abs(), p.conv), p.K, p.splitk, p.odt,
                           p.alpha, addends)
    if p.colsum:
        p.cs_ref = _d(p.colsum_prev) + A.sum(0)
        p.cs_bound = 2.0 * (p.K + p.splitk + 8) * U32 * (_d(p.colsum_prev).abs() + A.abs().sum(0))
    return p._ref


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite."""
    err = (_d(got) - ref).abs() / bound.clamp_min(1e-300)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return err.max().item()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def check(p, cb, cv, sb=None, sv=None, label=None):
    """The three assertions of every comparison: finite, sentinels bit-unchanged, max error / bound <= 1.  Returns the ratio
    (the larger of C's and colsum_out's); with a label the figures are printed as a GEMM_PARITY line BEFORE anything is asserted."""
    ref, bound = reference(p)
    if p.accumulate == 2:
        n = p.splitk * p.M * p.N
        intact = torch.equal(_bits(cb[n:]), _bits(p.C_buf[n:]))
        got = _d(cb[:n]).reshape(p.splitk, p.M, p.N).sum(0)
    else:
        mask = torch.ones_like(cb, dtype=torch.bool)
        mask[:p.M, p.c_off:p.c_off + p.N] = False
        intact = torch.equal(_bits(cb)[mask], _bits(p.C_buf)[mask])
        got = cv
    finite = bool(torch.isfinite(got).all())
    r = ratio(got, ref, bound)
    if p.colsum:
        mask = torch.ones_like(sb, dtype=torch.bool)
        mask[8:8 + p.M] = False
        intact = intact and torch.equal(_bits(sb)[mask], _bits(p.colsum_buf)[mask])
        finite = finite and bool(torch.isfinite(sv).all())
        r = max(r, ratio(sv, p.cs_ref, p.cs_bound))
    if label is not None:
        print(f"GEMM_PARITY {label} err/bound={r:.3f} finite={int(finite)} sentinels={int(intact)}")
    assert finite, "non-finite output"
    assert intact, "sentinel values around the output were written"
    assert r <= 1.0, f"error / bound = {r:.3g} > 1"
    return r


# ---------------------------------------------------------------------------------------------------------------- yardstick
FAULTS = ("drop_last_k", "drop_chunk", "dup_split", "rowvec_neighbour", "short_bias", "residual_row", "alpha_bias",
          "ignore_prev", "early_bf16", "border_wrap", "ignore_conv_ld", "mode1_row")


def _gather(p, img, fault=None):
    """The [pixels, 9 ci] im2col matrix of the image (k = (tap, ci)) in img's dtype, by F.unfold on the virtual image."""
    c = p.conv
    if fault == "ignore_conv_ld":               # pixel q read at q * ci instead of q * conv_ld
        flat = p.img_buf.detach().cpu().flatten()[8:8 + c.b * c.hi * c.wi * c.ci]
        img = flat.reshape(-1, c.ci).to(img.dtype)
    xv, stride, pad = _virtual(_nchw(c, img), c.mode)
    H, W = xv.shape[2], xv.shape[3]
    if fault == "border_wrap":                  # right border: the tap beyond the row reads the next row's first pixel
        assert pad == 1
        xv = F.pad(xv, (1, 1, 1, 1))
        xv[:, :, 1:H, W + 1] = xv[:, :, 2:H + 1, 1]
        pad = 0
    if fault == "mode1_row":                    # odd Hi, stride 2: the bottom tap reads row Hi = the next image's first row
        assert c.mode == 1 and (c.hi & 1)
        nxt = torch.cat([xv[1:, :, :1], torch.zeros_like(xv[:1, :, :1])], 0)
        xv = F.pad(torch.cat([xv, nxt], 2), (1, 1, 1, 0))
        pad = 0
    cols = F.unfold(xv, 3, padding=pad, stride=stride)                    # [B, ci * 9, L], rows ordered (ci, tap)
    L = cols.shape[2]
    cols = cols.reshape(c.b, c.ci, 9, L).permute(0, 3, 2, 1)              # [B, L, tap, ci]
    if fault == "mode1_row":
        cols = cols.reshape(c.b, -1, c.wo, 9, c.ci)[:, :c.ho]
    return cols.reshape(c.b * c.ho * c.wo, 9 * c.ci)


def yardstick(p, fault=None):
    """fp32 torch with p.splitk partial sums, rounded once to the output type; `fault` plants one defect (FAULTS).  Returns
    (C [M, N] in the output type, colsum [M] fp32 or None)."""
    assert fault is None or fault in FAULTS, fault
    f32 = torch.float32
    A, B = p.A.detach().cpu().to(f32), p.B.detach().cpu().to(f32)
    conv_fault = fault if fault in ("border_wrap", "ignore_conv_ld", "mode1_row") else None
    if p.kind == "linear":
        L, Rm = A, B
    elif p.kind == "wgrad":
        L, Rm = A.t(), B.t()
    elif p.kind == "conv":
        L, Rm = _gather(p, A, conv_fault), B
    else:
        L, Rm = A.t(), _gather(p, B, conv_fault).t()
    K = p.K
    nk = (K + 63) // 64
    per = (nk + p.splitk - 1) // p.splitk * 64
    ranges = [(s * per, min(K, (s + 1) * per)) for s in range(p.splitk) if s * per < K]
    if fault == "drop_last_k":
        ranges[-1] = (ranges[-1][0], ranges[-1][1] - 1)
    total = torch.zeros(p.M, p.N, dtype=f32)
    for i, (k0, k1) in enumerate(ranges):
        keep = torch.ones(K, dtype=torch.bool)
        if fault == "drop_chunk" and i == 0:
            edge = k1 if len(ranges) > 1 else min(64, K)                 # a split boundary (a K-step boundary when unsplit)
            keep[edge - 8:edge] = False
        part = L[:, k0:k1][:, keep[k0:k1]] @ Rm[:, k0:k1][:, keep[k0:k1]].t()
        total = total + part
        if fault == "dup_split" and i == len(ranges) - 1:
            total = total + part
    y = p.alpha * total
    if fault == "early_bf16":
        y = y.to(torch.bfloat16).to(f32)
    rows = torch.arange(p.M)
    if p.bias is not None:
        b = p.bias.detach().cpu().clone()
        if fault == "short_bias":
            assert p.N % 8
            b[p.N - p.N % 8:] = 0.0
        y = y + (p.alpha * b if fault == "alpha_bias" else b)
    if p.rv is not None:
        img = rows // p.rows_per_b
        if fault == "rowvec_neighbour":
            img = img.clone()
            img[p.rows_per_b] = 0                                         # first row of image 1 takes image 0's vector
        y = y + p.rv.detach().cpu()[img]
    if p.R is not None:
        r = p.R.detach().cpu().to(f32)
        if fault == "residual_row":
            r = r.clone()
            r[p.M - 1] = r[p.M - 2]
        y = y + r
    if p.prev is not None and fault != "ignore_prev":
        y = y + p.prev.detach().cpu().to(f32)
    cs = None
    if p.colsum:
        cs = p.colsum_prev + A.sum(0)
    return y.to(p.odt), cs


def yardstick_ratio(p, fault=None):
    ref, bound = reference(p)
    y, cs = yardstick(p, fault)
    r = ratio(y, ref, bound)
    if p.colsum and fault is None:
        r = max(r, ratio(cs, p.cs_ref, p.cs_bound))
    return r
