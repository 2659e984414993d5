"""Skinny linears (csrc/skinny.hip: pdmk_skinny_gemm, pdmk_skinny_wgrad): every column and row tail, both row forms with their
zero-filled rows, every trip count of the K loop and of the wgrad item loop, the capped grid, the LDS limits, strided operands
and every dtype pair, against the same contraction in float64 on the CPU.

Launch rule (restated from skinny.hip by _fwd_rule / _wgrad_rule).  Forward: MR = 8 if M <= 8 else 16 rows are staged in LDS
(rows >= M zero-filled, MR * K * sizeof(x type) <= 65536 bytes); a wave owns NPW = 4 output columns per pass, a block has 4
waves, blocks = min(ceil(ceil(N / 4) / 4), 1024), a wave's column loop steps by 4 * blocks * NPW; a lane's K loop starts at
lane * CH and steps by 64 * CH (CH = 8 for bf16 weights, 4 for fp32).  Wgrad: one block per 8 weight rows (rows >= N leave the
item loop by `break`), 8 * K / 4 float4 items over 256 threads, 512 + M * K * sizeof(x type) <= 65536 bytes of LDS.
SKINNY lists, per dtype pair, the smallest shapes that reach each of these; test_table_reaches_every_loop_tail_and_guard checks
on a machine without a GPU that every shape reaches what it is listed for, and the GPU tests take their shapes from the table.

Exact inputs.  x, w, dy and the previous contents of y, dw, dbias are integers in [-4, 4] (exact in bf16), bias values are
integers or halves.  With K <= 2048 every fp32 partial sum is an integer or a multiple of 1/2 below 2^24 (the table test
bounds the largest), so summation order cannot matter and the fp32 result is the exact sum; a bf16 output is that sum rounded
once, to nearest even (from_f32<bf16> of common.h is the compiler's float -> __bf16 conversion, as .to(torch.bfloat16) is).
The comparison is torch.equal on every shape and form of the table.

Strides and canaries.  Every operand is a column slice of a wider buffer: ldx, ldw and lddw are the smallest multiples the
entry checks allow above K, ldy and lddy are odd.  Padding the kernels may read (columns >= K, rows >= M of x and dy, rows >= N
of w, bias entries past N) holds 1e6; padding they may write (columns of y past N, rows >= M, columns of dw past K) holds a
sentinel and must come back bit-identical.  The rows of dw after N and dbias past N hold -0.0 and are compared by bit pattern:
the wgrad adds to what it finds, a block stages zeros for the dy of rows past N, and -0.0 + 0.0 = +0.0 shows an add that a
finite sentinel would hide.

One realistic-values case per dtype pair and shape runs randn inputs against float64 at TOL / close() of test_kernels_gpu.py and
prints a SKINNY_PARITY line (profiles/skinny_encoder_parity.txt is a collected run); the fixture itself is checked first: the
same contraction in fp32 on the CPU is within half the bound.  (16, 321, 1280) with an fp32 skinny operand needs 80 KiB of LDS:
the entry points document <= 64 KiB, and the case asserts the refusal."""
import functools
import os
import re

import pytest
import torch

from test_kernels_gpu import DT, TOL, close

MMAX, NPW, WAVES, MAXBLK, NT = 16, 4, 4, 1024, 256
LDS_MAX = 64 * 1024
CH = {"bf16": 8, "f32": 4}
SZ = {"bf16": 2, "f32": 4}
PAIRS = (("bf16", "bf16"), ("bf16", "f32"), ("f32", "f32"))       # forward: (weight, skinny operand); wgrad: (x, dy)
SENT = -123.0                     # 7 significant bits: exact in bf16; no result of an exact-input case is checked against it
POISON = 1e6
ROWS_AFTER = 8                    # dw / dbias rows after N: a block's 8 rows stay inside the buffer whatever the kernel does
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unlearn-ft_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the launch rule
def _fwd_rule(M, N, K, wdn, xdn):
    ch = CH[wdn]
    mr = 8 if M <= 8 else 16
    waves = -(-N // NPW)
    blocks = max(1, min(-(-waves // WAVES), MAXBLK))
    per_pass = blocks * WAVES
    passes = -(-waves // per_pass)
    return dict(MR=mr, CH=ch, waves=waves, blocks=blocks, per_pass=per_pass, passes=passes,
                last_pass_waves=waves - (passes - 1) * per_pass, tail=N % NPW, chunks=K // ch, lds=mr * K * SZ[xdn])


def _wgrad_rule(M, N, K, xdn):
    return dict(blocks=-(-N // 8), items=8 * (K // 4), row_tail=N % 8, lds=8 * MMAX * 4 + M * K * SZ[xdn])


_N_WHY = {1: ("tail1", "n_lt_npw", "idle_waves"), 3: ("tail3", "n_lt_npw", "idle_waves"), 5: ("tail1", "idle_waves"),
          6: ("tail2", "idle_waves"), 13: ("tail1", "full_block")}


def _fwd_shapes(wdn, xdn):
    ch = CH[wdn]
    # K = 1280 goes with 16 staged rows where they fit the LDS (bf16 operand), else with 8 (fp32: 16 x 1280 x 4 bytes = 80 KiB)
    k8, k9 = (65 * ch, 1280) if xdn == "bf16" else (1280, 65 * ch)
    kw = {65 * ch: "k_second_trip", 1280: "k_1280"}
    mk = [(1, ch, ("mr8_zero_rows", "k_one_lane")), (7, 64 * ch, ("mr8_zero_rows", "k_one_trip")),
          (8, k8, ("mr8_full", kw[k8])), (9, k9, ("mr16_zero_rows", kw[k9])),
          (16, 65 * ch, ("mr16_full", "k_second_trip"))]
    out = [dict(M=M, N=N, K=K, why=_N_WHY[N] + why) for N in _N_WHY for M, K, why in mk]
    out.append(dict(M=3, N=16 * 1024 + 4 * 5 + 3, K=ch, why=("two_passes_ragged", "tail3", "mr8_zero_rows", "k_one_lane")))
    out.append(dict(M=16 if xdn == "bf16" else 8, N=5, K=2048, why=("lds_limit",)))
    return out


def _wgrad_shapes(xdn):
    k_why = {4: "one_item_per_row", 128: "one_trip", 132: "ragged_second_trip"}
    out = []
    for i, N in enumerate((1, 7, 9, 13)):
        for j, K in enumerate(k_why):
            M = (1, 3, 16)[(i + j) % 3]
            out.append(dict(M=M, N=N, K=K, why=("row_tail", k_why[K], f"m{M}") + (("two_blocks",) if N > 8 else ("one_block",))))
    out.append(dict(M=16 if xdn == "bf16" else 8, N=9, K=2032, why=("lds_limit", "row_tail")))
    return out


# (kind, (first type, second type), shape): forward pairs are (weight, skinny operand), wgrad pairs are (x, dy)
SKINNY = ([("fwd", pr, p) for pr in PAIRS for p in _fwd_shapes(*pr)]
          + [("wgrad", pr, p) for pr in PAIRS for p in _wgrad_shapes(pr[0])])

_FWD_REACHES = {
    "tail1": lambda p, r: r["tail"] == 1, "tail2": lambda p, r: r["tail"] == 2, "tail3": lambda p, r: r["tail"] == 3,
    "n_lt_npw": lambda p, r: p["N"] < NPW and r["waves"] == 1,
    "idle_waves": lambda p, r: r["passes"] == 1 and r["blocks"] * WAVES > r["waves"],
    "full_block": lambda p, r: r["passes"] == 1 and r["blocks"] * WAVES == r["waves"],
    "mr8_zero_rows": lambda p, r: r["MR"] == 8 and p["M"] < 8, "mr8_full": lambda p, r: p["M"] == 8 and r["MR"] == 8,
    "mr16_zero_rows": lambda p, r: r["MR"] == 16 and p["M"] < 16, "mr16_full": lambda p, r: p["M"] == 16,
    "k_one_lane": lambda p, r: r["chunks"] == 1, "k_one_trip": lambda p, r: r["chunks"] == 64,
    "k_second_trip": lambda p, r: r["chunks"] == 65,            # lane 0 alone takes a second trip
    "k_1280": lambda p, r: p["K"] == 1280 and r["chunks"] in (160, 320),    # bf16: lanes 0-31 three trips, 32-63 two; fp32: five
    # the capped grid: two passes, the second one with fewer waves than the grid, its last block partly filled, its last
    # wave with a column tail; the weight (with its padding) stays under 1 MiB
    "two_passes_ragged": lambda p, r: (r["blocks"] == MAXBLK and r["passes"] == 2 and 0 < r["last_pass_waves"] < r["per_pass"]
                                       and r["last_pass_waves"] % WAVES and r["tail"] == 3),
    "lds_limit": lambda p, r: r["lds"] == LDS_MAX,
}
_WGRAD_REACHES = {
    "row_tail": lambda p, r: r["row_tail"] != 0, "one_block": lambda p, r: r["blocks"] == 1,
    "two_blocks": lambda p, r: r["blocks"] == 2, "one_item_per_row": lambda p, r: r["items"] == 8,
    "one_trip": lambda p, r: r["items"] == NT, "ragged_second_trip": lambda p, r: NT < r["items"] < 2 * NT,
    "m1": lambda p, r: p["M"] == 1, "m3": lambda p, r: p["M"] == 3, "m16": lambda p, r: p["M"] == 16,
    "lds_limit": lambda p, r: r["lds"] == LDS_MAX,
}
REALISTIC = ((8, 1283, 320), (16, 321, 1280))


def _id(a):
    if isinstance(a, dict):
        return f"M{a['M']}-N{a['N']}-K{a['K']}"
    return "-".join(a) if isinstance(a, tuple) else str(a)


def _table(kind):
    return [(pr, p) for k_, pr, p in SKINNY if k_ == kind]


# ------------------------------------------------------------------------------------------------ host-only checks
def test_table_reaches_every_loop_tail_and_guard():
    """Host only: every shape of SKINNY reaches what it is listed for, every pair has every listed form, and the exact-arithmetic
    bound holds."""
    seen = {}
    for kind, pr, p in SKINNY:
        M, N, K = p["M"], p["N"], p["K"]
        if kind == "fwd":
            r, reaches = _fwd_rule(M, N, K, *pr), _FWD_REACHES
            assert K % r["CH"] == 0 and r["lds"] <= LDS_MAX, (kind, pr, p)
        else:
            r, reaches = _wgrad_rule(M, N, K, pr[0]), _WGRAD_REACHES
            assert K % 4 == 0 and r["lds"] <= LDS_MAX, (kind, pr, p)
        assert 1 <= M <= MMAX and p["why"], (kind, pr, p)
        for why in p["why"]:
            assert reaches[why](p, r), (kind, pr, _id(p), why, r)
            seen.setdefault((kind, pr), set()).add(why)
        if "lds_limit" in p["why"]:         # one chunk more is past the limit
            more = _fwd_rule(M, N, K + CH[pr[0]], *pr) if kind == "fwd" else _wgrad_rule(M, N, K + 4, pr[0])
            assert more["lds"] > LDS_MAX, (kind, pr, p)
        if "two_passes_ragged" in p["why"]:
            assert N == 16 * 1024 + 4 * 5 + 3 and r["last_pass_waves"] == 6 and N * (K + r["CH"]) * SZ[pr[0]] < 2 ** 20
    for pr in PAIRS:
        assert seen[("fwd", pr)] == set(_FWD_REACHES), (pr, set(_FWD_REACHES) - seen[("fwd", pr)])
        assert seen[("wgrad", pr)] == set(_WGRAD_REACHES), (pr, set(_WGRAD_REACHES) - seen[("wgrad", pr)])
        assert {p["M"] for p in _fwd_shapes(*pr)} >= {1, 3, 7, 8, 9, 16}
        assert {p["K"] for p in _fwd_shapes(*pr)} >= {CH[pr[0]], 64 * CH[pr[0]], 65 * CH[pr[0]], 1280, 2048}
    # exact arithmetic: |x|, |w|, |dy| <= 4, previous contents <= 4, |bias| <= 4: the largest |sum| is an integer or a half
    # below 2^24, so every fp32 partial sum is exact in any order
    kmax = max(p["K"] for _, _, p in SKINNY)
    assert kmax <= 2048 and kmax * 16 + 4 + 4 == 32776 and 32776 < 2 ** 24
    assert MMAX * 16 + 4 < 2 ** 24                                  # wgrad: a sum over M <= 16 rows


def test_restated_constants_are_the_sources():
    """Host only: the constants the table is built from are the ones in skinny.hip (a changed cap, tile or limit there must be
    followed here, or the table no longer reaches what it lists)."""
    src = open(os.path.join(CSRC, "skinny.hip")).read()
    assert re.search(r"constexpr int MMAX = 16;", src) and re.search(r"constexpr int NPW = 4;", src)
    assert "const int MR = M <= 8 ? 8 : 16;" in src and "min((waves + 3) / 4, 1024)" in src
    assert "const int gw = blockIdx.x * 4 + wave, nwaves = gridDim.x * 4;" in src
    assert "n0 += nwaves * NPW" in src and "k0 += 64 * CH" in src
    assert src.count("if (shm > 64 * 1024) return -1;") == 2 and "8 * MMAX * 4 + (size_t)M * K * sizeof(T)" in src
    assert "dim3((N + 7) / 8), dim3(256)" in src and "i < 8 * kq; i += 256" in src


@functools.lru_cache(maxsize=None)
def _realistic(M, N, K, wdn, xdn):
    """CPU tensors of one realistic-values case: x, dy ~ N(0, 1), w ~ N(0, 1 / K), rounded to their types; fp64 references"""
    g = torch.Generator().manual_seed(M * 7919 + N)
    x = torch.randn(M, K, generator=g).to(DT[xdn])
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DT[wdn])
    bias = torch.randn(N, generator=g)
    ref = x.double() @ w.double().t() + bias.double()
    ref32 = x.float() @ w.float().t() + bias
    return x, w, bias, ref, ref32


@functools.lru_cache(maxsize=None)
def _realistic_wgrad(M, N, K, xdn, dydn):
    g = torch.Generator().manual_seed(M * 7919 + N + 1)
    x = torch.randn(M, K, generator=g).to(DT[xdn])
    dy = (torch.randn(M, N, generator=g) * K ** -0.5).to(DT[dydn])
    dw0, db0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    ref = (dw0.double() + dy.double().t() @ x.double(), db0.double() + dy.double().sum(0))
    ref32 = (dw0 + dy.float().t() @ x.float(), db0 + dy.float().sum(0))
    return x, dy, dw0, db0, ref, ref32


def _check_fixture(M, N, K, pr):
    """The fixture condition of the realistic-values cases: the fp32 restatement on the CPU is within half the bound"""
    tol = TOL[pr[0]]
    _, _, _, ref, ref32 = _realistic(M, N, K, *pr)
    for ydt in {torch.float32, DT[pr[0]]}:
        close(ref32.to(ydt), ref, tol / 2, f"fixture fwd {pr} {ydt}")
    _, _, _, _, wref, wref32 = _realistic_wgrad(M, N, K, *pr)
    close(wref32[0], wref[0], tol / 2, f"fixture wgrad {pr}")
    close(wref32[1], wref[1], tol / 2, f"fixture dbias {pr}")


@pytest.mark.parametrize("pr", PAIRS, ids=_id)
@pytest.mark.parametrize("M,N,K", REALISTIC)
def test_realistic_fixture_fp32_is_within_half_the_bound(M, N, K, pr):
    """Host only"""
    _check_fixture(M, N, K, pr)


# ------------------------------------------------------------------------------------------------ helpers of the GPU tests
def _ints(shape, g, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def _read_buf(vals, rows, ld, dt, dev):
    """vals [r, c] (fp64, CPU) as the top-left corner of a [rows, ld] device buffer whose other elements hold 1e6"""
    buf = torch.full((rows, ld), POISON, dtype=torch.float64)
    buf[:vals.shape[0], :vals.shape[1]] = vals
    buf = buf.to(dt).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf


def _write_buf(vals, rows, ld, dt, dev):
    """vals [r, c] as the top-left corner of a [rows, ld] device buffer whose other elements hold the sentinel"""
    buf = torch.full((rows, ld), SENT, dtype=torch.float64)
    buf[:vals.shape[0], :vals.shape[1]] = vals
    buf = buf.to(dt).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf


def _pads_intact(buf, r, c, what):
    assert bool((buf[:r, c:] == SENT).all()), what + ": padding columns written"
    assert bool((buf[r:] == SENT).all()), what + ": rows after the last written"


def _wgrad_pads_intact(dwbuf, dbbuf, N, K, what):
    assert bool((dwbuf[:N, K:] == SENT).all()), what + ": padding columns of dw written"
    assert bool((dwbuf[N:].contiguous().view(torch.int32) == -2 ** 31).all()), what + ": rows of dw after N written"
    assert bool((dbbuf[N:].contiguous().view(torch.int32) == -2 ** 31).all()), what + ": dbias written past N"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _odd_above(n):
    return n + 1 + (n % 2)


def _fwd_operands(M, N, K, wdn, xdn, dev, vals=None, seed=0):
    """(x64, w64, bias64, y0_64, xbuf, wbuf, biasbuf, ldx, ldw, ldy): exact integer values unless `vals` gives (x, w, bias)"""
    g = torch.Generator().manual_seed(seed * 1000003 + M * 131 + N * 17 + K)
    if vals is None:
        x64, w64, b64 = _ints((M, K), g), _ints((N, K), g), _ints((N,), g, -8, 8) / 2
    else:
        x64, w64, b64 = (v.double() for v in vals)
    y0 = _ints((M, N), g)
    ldx, ldw, ldy = K + 4, K + CH[wdn], _odd_above(N)
    assert ldx % 4 == 0 and ldw % CH[wdn] == 0 and ldy % 2 == 1
    xbuf = _read_buf(x64, MMAX, ldx, DT[xdn], dev)
    wbuf = _read_buf(w64, N + NPW, ldw, DT[wdn], dev)
    bbuf = _read_buf(b64.view(1, N), 1, N + 8, torch.float32, dev).view(-1)
    return x64, w64, b64, y0, xbuf, wbuf, bbuf, ldx, ldw, ldy


def _out_types(wdn):
    return (torch.float32,) if wdn == "f32" else (torch.float32, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.gpu
@pytest.mark.parametrize("pr,p", _table("fwd"), ids=_id)
def test_skinny_gemm_exact(dev, pr, p):
    """Every output type, accumulate off and on, bias absent and present (bias with accumulate: y_old + x w^T + bias)"""
    from pdm import _pdmk as k
    M, N, K = p["M"], p["N"], p["K"]
    wdn, xdn = pr
    x64, w64, b64, y0, xbuf, wbuf, bbuf, ldx, ldw, ldy = _fwd_operands(M, N, K, wdn, xdn, dev)
    base = x64 @ w64.t()
    assert float(base.abs().max()) + 8 < 2 ** 24
    for ydt in _out_types(wdn):
        for acc in (False, True):
            for with_bias in (False, True):
                what = f"skinny_gemm w={wdn} x={xdn} {_id(p)} y={ydt} acc={acc} bias={with_bias}"
                ybuf = _write_buf(y0, MMAX + 1, ldy, ydt, dev)
                k.skinny_gemm(xbuf, wbuf, ybuf, M, N, K, ldx, ldw, ldy, bias=bbuf if with_bias else None, accumulate=acc)
                ref = base + (b64 if with_bias else 0.0) + (y0 if acc else 0.0)
                got = ybuf[:M, :N].cpu()
                assert torch.equal(got, ref.to(ydt)), f"{what}: {int((got != ref.to(ydt)).sum())} of {M * N} elements differ"
                _pads_intact(ybuf, M, N, what)


@pytest.mark.gpu
@pytest.mark.parametrize("pr", PAIRS, ids=_id)
def test_skinny_gemm_lds_limit_refused(dev, pr):
    """One chunk past the LDS limit: PdmkError, y bit-identical"""
    from pdm import _pdmk as k
    wdn, xdn = pr
    p = [q for q in _fwd_shapes(wdn, xdn) if "lds_limit" in q["why"]][0]
    M, N, K = p["M"], p["N"], p["K"] + CH[wdn]
    assert _fwd_rule(M, N, K, wdn, xdn)["lds"] > LDS_MAX
    _, _, _, y0, xbuf, wbuf, bbuf, ldx, ldw, ldy = _fwd_operands(M, N, K, wdn, xdn, dev)
    for ydt in _out_types(wdn):
        ybuf = _write_buf(y0, MMAX + 1, ldy, ydt, dev)
        before = ybuf.clone()
        with pytest.raises(k.PdmkError):
            k.skinny_gemm(xbuf, wbuf, ybuf, M, N, K, ldx, ldw, ldy, bias=bbuf)
        torch.cuda.synchronize()
        assert torch.equal(ybuf, before)


# ------------------------------------------------------------------------------------------------ wgrad
def _wgrad_operands(M, N, K, xdn, dydn, dev, vals=None):
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K + 5)
    if vals is None:
        x64, dy64, dw0, db0 = _ints((M, K), g), _ints((M, N), g), _ints((N, K), g), _ints((N,), g)
    else:
        x64, dy64, dw0, db0 = (v.double() for v in vals)
    ldx, lddy, lddw = K + 4, _odd_above(N), K + 4
    xbuf = _read_buf(x64, MMAX, ldx, DT[xdn], dev)
    dybuf = _read_buf(dy64, MMAX, lddy, DT[dydn], dev)
    nrows = -(-N // 8) * 8 + ROWS_AFTER
    dwbuf = _write_buf(dw0, nrows, lddw, torch.float32, dev)
    dbbuf = _write_buf(db0.view(1, N), 1, nrows, torch.float32, dev).view(-1)
    dwbuf[N:] = -0.0                  # what the kernel adds to is checked by bit pattern: -0.0 + 0.0 is +0.0, so a block that
    dbbuf[N:] = -0.0                  # adds zeros to the rows after N (their dy is staged as zero) still shows
    return x64, dy64, dw0, db0, xbuf, dybuf, dwbuf, dbbuf, ldx, lddy, lddw


@pytest.mark.gpu
@pytest.mark.parametrize("pr,p", _table("wgrad"), ids=_id)
def test_skinny_wgrad_exact(dev, pr, p):
    """dw and dbias are added to (both pre-filled); dbias present and None"""
    from pdm import _pdmk as k
    M, N, K = p["M"], p["N"], p["K"]
    xdn, dydn = pr
    for with_db in (True, False):
        x64, dy64, dw0, db0, xbuf, dybuf, dwbuf, dbbuf, ldx, lddy, lddw = _wgrad_operands(M, N, K, xdn, dydn, dev)
        what = f"skinny_wgrad x={xdn} dy={dydn} {_id(p)} dbias={with_db}"
        k.skinny_wgrad(dybuf, xbuf, dwbuf, dbbuf if with_db else None, M, N, K, lddy, ldx, lddw)
        ref = dw0 + dy64.t() @ x64
        got = dwbuf[:N, :K].cpu()
        assert torch.equal(got, ref.float()), f"{what}: {int((got != ref.float()).sum())} of {N * K} elements of dw differ"
        dbref = db0 + (dy64.sum(0) if with_db else 0.0)
        assert torch.equal(dbbuf[:N].cpu(), dbref.float()), what + " dbias"
        _wgrad_pads_intact(dwbuf, dbbuf, N, K, what)


@pytest.mark.gpu
@pytest.mark.parametrize("pr", PAIRS, ids=_id)
def test_skinny_wgrad_lds_limit_refused(dev, pr):
    from pdm import _pdmk as k
    xdn, dydn = pr
    p = [q for q in _wgrad_shapes(xdn) if "lds_limit" in q["why"]][0]
    M, N, K = p["M"], p["N"], p["K"] + 4
    assert _wgrad_rule(M, N, K, xdn)["lds"] > LDS_MAX
    _, _, _, _, xbuf, dybuf, dwbuf, dbbuf, ldx, lddy, lddw = _wgrad_operands(M, N, K, xdn, dydn, dev)
    before = _bits(dwbuf).clone(), _bits(dbbuf).clone()
    with pytest.raises(k.PdmkError):
        k.skinny_wgrad(dybuf, xbuf, dwbuf, dbbuf, M, N, K, lddy, ldx, lddw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dwbuf), before[0]) and torch.equal(_bits(dbbuf), before[1])


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refused_calls_leave_outputs_untouched(dev):
    """Every argument check of the two entry points, one argument off a call that is accepted: status -1 (-2 for fp32 weights
    with a bf16 operand), and nothing written"""
    from pdm import _pdmk as k
    g = torch.Generator().manual_seed(11)
    M, N = 4, 6
    outs = []

    def out(n, dt):
        t = torch.full((n,), SENT, device=dev, dtype=dt)
        outs.append(t)
        return t

    for wdn, xdn in PAIRS:
        ch = CH[wdn]
        K = 2 * ch
        ldx, ldw, ldy = K + 4, K + ch, N + 1
        x = _ints((MMAX * ldx + 8,), g).to(DT[xdn]).to(dev)
        w = _ints(((N + 4) * (ldw + ch) + 8,), g).to(DT[wdn]).to(dev)
        bias = _ints((N,), g).float().to(dev)

        def fwd(x_=x, w_=w, M_=M, N_=N, K_=K, ldx_=ldx, ldw_=ldw, y_=None):
            y_ = out((MMAX + 1) * ldy, torch.float32) if y_ is None else y_
            return k._lib.pdmk_skinny_gemm(k._p(x_), k.dt(x_), k._p(w_), k._p(y_), k._p(bias), M_, N_, K_, ldx_, ldw_, ldy, k.dt(w_),
                                           1, 0, k._st())

        assert fwd(y_=torch.empty((MMAX + 1) * ldy, device=dev)) == 0            # the call every refusal is one argument off
        assert fwd(M_=0) == -1 and fwd(M_=MMAX + 1) == -1 and fwd(N_=0) == -1 and fwd(K_=0) == -1
        assert fwd(K_=K + ch // 2) == -1, "K not a multiple of CH"
        assert fwd(ldw_=ldw + ch // 2) == -1, "ldw not a multiple of CH"
        assert fwd(ldx_=ldx + 2) == -1, "ldx not a multiple of 4"
        assert fwd(w_=w[1:]) == -1 and fwd(x_=x[1:]) == -1, "misaligned w, x"
        yo = out((MMAX + 1) * ldy, torch.float32)
        assert k._lib.pdmk_skinny_gemm(None, k.dt(x), k._p(w), k._p(yo), None, M, N, K, ldx, ldw, ldy, k.dt(w), 1, 0, k._st()) == -1
        with pytest.raises(k.PdmkError):
            k.skinny_gemm(x, w, out((MMAX + 1) * ldy, torch.float32), MMAX + 1, N, K, ldx, ldw, ldy)

        # wgrad: (x type, dy type) = (wdn, xdn) of this pair
        xg = _ints((MMAX * ldx + 8,), g).to(DT[wdn]).to(dev)
        dy = _ints((MMAX * (N + 1) + 8,), g).to(DT[xdn]).to(dev)
        lddw = K + 4

        def wgrad(M_=M, N_=N, K_=K, ldx_=ldx, lddw_=lddw, dw_=None, off=0):
            db_ = out(N + ROWS_AFTER, torch.float32) if dw_ is None else torch.zeros(N + ROWS_AFTER, device=dev)
            dw_ = out((N + 2 + ROWS_AFTER) * (lddw + 4) + 4, torch.float32) if dw_ is None else dw_
            return k._lib.pdmk_skinny_wgrad(k._p(dy), k.dt(dy), k._p(xg), k._p(dw_[off:]), k._p(db_), M_, N_, K_, N + 1, ldx_, lddw_,
                                            k.dt(xg), k._st())

        assert wgrad(dw_=torch.zeros((N + 2 + ROWS_AFTER) * (lddw + 4) + 4, device=dev)) == 0
        assert wgrad(M_=0) == -1 and wgrad(M_=MMAX + 1) == -1 and wgrad(N_=0) == -1 and wgrad(K_=0) == -1
        assert wgrad(K_=K + 2) == -1, "K not a multiple of 4"
        assert wgrad(lddw_=lddw + 2) == -1, "lddw not a multiple of 4"
        assert wgrad(ldx_=ldx + 2) == -1, "ldx not a multiple of 4"
        assert wgrad(off=1) == -1, "misaligned dw"
    # fp32 weights with a bf16 operand: -2, from both entry points
    wf = _ints((64,), g).float().to(dev)
    xb = _ints((64,), g).to(torch.bfloat16).to(dev)
    assert k._lib.pdmk_skinny_gemm(k._p(xb), k.BF16, k._p(wf), k._p(out(64, torch.float32)), None, 2, 2, 8, 8, 8, 2, k.F32, 1, 0,
                                   k._st()) == -2
    assert k._lib.pdmk_skinny_wgrad(k._p(xb), k.BF16, k._p(wf), k._p(out(64, torch.float32)), k._p(out(8, torch.float32)), 2, 2, 8, 2,
                                    8, 8, k.F32, k._st()) == -2
    with pytest.raises(k.PdmkError):
        k.skinny_gemm(xb, wf, out(64, torch.float32), 2, 2, 8, 8, 8, 2)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENT).all()), "a refused call wrote its output"


# ------------------------------------------------------------------------------------------------ realistic values
def _parity(entry, pr, shape, got, ref, tol):
    """One SKINNY_PARITY line, then the project's whole-tensor check (max error and relative L2 error against `tol`)"""
    got = got.double().cpu()
    err = float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-6)
    l2 = float((got - ref).norm()) / (float(ref.norm()) + 1e-30)
    print(f"SKINNY_PARITY {entry} {pr[0]}/{pr[1]} {shape} err={err:.3e} l2={l2:.3e} tol={tol:.1e}")
    close(got, ref, tol, f"{entry} {pr} {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("pr", PAIRS, ids=_id)
@pytest.mark.parametrize("M,N,K", REALISTIC)
def test_skinny_realistic_values(dev, M, N, K, pr):
    """randn inputs, strided, against fp64 on the rounded inputs at TOL.  Where the skinny operand does not fit the documented
    64 KiB of LDS ((16, 321, 1280) with an fp32 operand) the entry point must refuse the call and write nothing."""
    from pdm import _pdmk as k
    _check_fixture(M, N, K, pr)
    tol, shape = TOL[pr[0]], f"M={M} N={N} K={K}"
    x, w, bias, ref, _ = _realistic(M, N, K, *pr)
    _, _, _, y0, xbuf, wbuf, bbuf, ldx, ldw, ldy = _fwd_operands(M, N, K, pr[0], pr[1], dev, vals=(x, w, bias))
    fits = _fwd_rule(M, N, K, *pr)["lds"] <= LDS_MAX
    for ydt in _out_types(pr[0]):
        ybuf = _write_buf(y0, MMAX + 1, ldy, ydt, dev)
        if not fits:
            before = ybuf.clone()
            with pytest.raises(k.PdmkError):
                k.skinny_gemm(xbuf, wbuf, ybuf, M, N, K, ldx, ldw, ldy, bias=bbuf)
            torch.cuda.synchronize()
            assert torch.equal(ybuf, before)
            continue
        k.skinny_gemm(xbuf, wbuf, ybuf, M, N, K, ldx, ldw, ldy, bias=bbuf)
        _parity("gemm_" + ("f32" if ydt == torch.float32 else "bf16") + "out", pr, shape, ybuf[:M, :N], ref, tol)
        _pads_intact(ybuf, M, N, f"skinny_gemm {pr} {shape}")
    xg, dy, dw0, db0, wref, _ = _realistic_wgrad(M, N, K, *pr)
    _, _, _, _, xbuf, dybuf, dwbuf, dbbuf, ldx, lddy, lddw = _wgrad_operands(M, N, K, pr[0], pr[1], dev, vals=(xg, dy, dw0, db0))
    if _wgrad_rule(M, N, K, pr[0])["lds"] > LDS_MAX:
        before = _bits(dwbuf).clone(), _bits(dbbuf).clone()
        with pytest.raises(k.PdmkError):
            k.skinny_wgrad(dybuf, xbuf, dwbuf, dbbuf, M, N, K, lddy, ldx, lddw)
        torch.cuda.synchronize()
        assert torch.equal(_bits(dwbuf), before[0]) and torch.equal(_bits(dbbuf), before[1])
        return
    k.skinny_wgrad(dybuf, xbuf, dwbuf, dbbuf, M, N, K, lddy, ldx, lddw)
    _parity("wgrad_dw", pr, shape, dwbuf[:N, :K], wref[0], tol)
    _parity("wgrad_dbias", pr, shape, dbbuf[:N], wref[1], tol)
    _wgrad_pads_intact(dwbuf, dbbuf, N, K, f"skinny_wgrad {pr} {shape}")
