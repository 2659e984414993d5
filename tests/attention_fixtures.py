"""Fixtures, references and yardsticks for the attention kernel tests (pure torch, CPU or GPU; not a conftest).

Inputs.  With randn Q / K the softmax over thousands of keys is flat: every output row is close to the mean of V, a
misaddressed key moves it by a few times the bf16 rounding, and the online softmax never rescales a non-zero accumulator.
The fixtures here PLANT a dominant key per query:

    k = randn,   q_i = a * k[pi(i)] + 0.5 * randn,   v, dO = randn,   everything rounded to the compute dtype

`pi` is a seeded surjection of the queries onto the keys that is not the identity (a permuted i mod Nk; it hits the first
and last key of every 64-key block and the very last key).  The gain `a` sets how peaked a row is.  With |k|^2 ~ 64 and
scale = 1/8 the planted score is ~ 8a and the other scores are N(0, a^2 + 1/4), so the row-maximum probability is about

    p = sigmoid(8a - (a^2 + 1/4) / 2 - ln(Nk - 1))

and planted_gain() solves that for a target p: "peaked" aims at 0.93 (band 0.85-0.98: single keys / V rows decide `o`,
single queries decide `dv`), "mid" at 0.5 (band 0.3-0.7: dS = P (dP - delta) is far from zero, `dq` / `dk` are sensitive).
tests/test_attention_host.py asserts the bands and the sensitivities on the fp64 reference alone.

The RESCALE variant aims at the forward's lazy online-softmax reference, which only moves when a key block's maximum exceeds it
by more than 8 (base 2): rows whose planted key sits in the last key block (move late, over non-zero accumulators), rows with a
weakly planted key after the first block (exceed the reference by 4-8: it must NOT move, probabilities up to 2^8), rows with
two planted keys of rising strength (stay, then move), and ordinary peaked rows.

References are fp64 (autograd backward), one (b, h) slice at a time.  Yardsticks are the same tensors from an honest
computation in each dtype's rounding policy: torch fp32 for fp32; for bf16 a "policy twin" of the kernels' header comment: bf16
inputs, fp32 scores and statistics, probabilities rounded to bf16 ONCE before every product that consumes them (the row sum
included: numerator and denominator of `o` see the same rounded P), dS rounded to bf16 likewise, fp32 accumulation, bf16 outputs.
A kernel passes when its error against fp64 is at most FACTOR x the yardstick's own error (floor: 8 ulp at the tensor's maximum)."""
import math

import torch

D = 64
SCALE = D ** -0.5
LOG2E = 1.4426950408889634
KVB = {torch.bfloat16: 64, torch.float32: 32}       # key rows per streamed block of the forward / dQ kernels
PMAX_BAND = {"peaked": (0.85, 0.98), "mid": (0.3, 0.7)}
PMAX_TARGET = {"peaked": 0.93, "mid": 0.5}
FACTOR = 8.0                                        # kernel error <= FACTOR x yardstick error (the FID tests' factor)
TENSORS = ("o", "lse", "dq", "dk", "dv")
STATS = ("max", "l2", "row")


def planted_gain(Nk, target):
    """The gain `a` for which a planted row's maximum probability is about `target` among Nk keys (module docstring)."""
    if Nk <= 1:
        return 1.0
    want = math.log(target / (1.0 - target)) + math.log(Nk - 1)
    lo, hi = 0.0, 6.0                               # 8a - a^2/2 rises on [0, 8)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if 8.0 * mid - 0.5 * (mid * mid + 0.25) < want:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def required_keys(Nk):
    """Keys `pi` must hit: the first and last key of every 64-key block, and the very last key."""
    req = set()
    for b0 in range(0, Nk, 64):
        req.add(b0)
        req.add(min(b0 + 63, Nk - 1))
    req.add(Nk - 1)
    return sorted(req)


def planted_pi(Nq, Nk, g, causal=False):
    """Seeded map query -> planted key.  Non-causal: sigma(i mod Nk) for a random permutation sigma (a surjection when
    Nq >= Nk; otherwise the required keys are forced onto the first queries).  Causal: a random key <= i, the last query on
    the last key."""
    i = torch.arange(Nq)
    if causal:
        assert Nq == Nk
        r = torch.randint(0, 1 << 30, (Nq,), generator=g)
        pi = i - r % (i + 1)
        pi[Nq - 1] = Nk - 1
        if Nq > 2 and bool((pi == i).all()):
            pi[Nq - 2] = 0
        return pi
    sigma = torch.randperm(Nk, generator=g)
    pi = sigma[i % Nk]
    if Nq < Nk:
        req = torch.tensor(required_keys(Nk))[:Nq]
        pi[:len(req)] = req
    if Nq > 1 and bool((pi == i).all()):
        pi = pi.roll(1)
    return pi


class Fixture:
    """q, do: [B, H, Nq, 64]; k, v: [B, H, Nk, 64] in `dtype` (CPU); pi: [Nq] planted key (-1: none); gain: the `a` used."""

    def __init__(self, kind, q, k, v, do, pi, gain, causal=False):
        self.kind, self.q, self.k, self.v, self.do, self.pi, self.gain, self.causal = kind, q, k, v, do, pi, gain, causal
        self.B, self.H, self.Nq, _ = q.shape
        self.Nk = k.shape[2]
        self.dtype = q.dtype

    def slice(self, b, h, device=None):
        t = tuple(x[b, h] for x in (self.q, self.k, self.v, self.do))
        return t if device is None else tuple(x.to(device) for x in t)


def _slice_gen(seed, B, H, b, h):
    """Every (b, h) slice draws from its own stream, so a fixture at a reduced B * H is the leading slices of the full one."""
    return torch.Generator().manual_seed(seed * 1000003 + b * 4099 + h)


def _draw(seed, B, H, Nq, Nk, make_q):
    q, k, v, do = (torch.empty(B, H, n, D) for n in (Nq, Nk, Nk, Nq))
    for b in range(B):
        for h in range(H):
            g = _slice_gen(seed, B, H, b, h)
            k[b, h] = torch.randn(Nk, D, generator=g)
            q[b, h] = make_q(k[b, h]) + 0.5 * torch.randn(Nq, D, generator=g)
            v[b, h] = torch.randn(Nk, D, generator=g)
            do[b, h] = torch.randn(Nq, D, generator=g)
    return q, k, v, do


def make_planted(B, H, Nq, Nk, regime, dtype, seed, causal=False):
    pi = planted_pi(Nq, Nk, torch.Generator().manual_seed(seed), causal)
    # causal: the median row sees about half of the keys
    a = planted_gain(max(2, Nk // 2) if causal else Nk, PMAX_TARGET[regime])
    q, k, v, do = _draw(seed, B, H, Nq, Nk, lambda ks: a * ks[pi])
    return Fixture(regime, q.to(dtype), k.to(dtype), v.to(dtype), do.to(dtype), pi, a, causal)


RESCALE_GAINS = {"late": 1.5, "under": 0.75, "stairs": (1.2, 2.2), "plain": 1.5}


def make_rescale(B, H, Nq, Nk, dtype, seed):
    """Rows by i mod 20: 7 "late" (a = 1.5, key in the last 32 keys' block), 5 "under" (a = 0.75, key after the first 64), 5 "stairs"
    (a = 1.2 in a middle 64-key block, then 2.2 in a later one), 3 "plain" (a = 1.5, any key).  Reasoning in base 2 (x 1.44):
    planted score ~ 11.5 a, largest other score of a 64-key block ~ 3.5 sqrt(sum a^2 + 1/4) - late rows exceed the first block's
    reference by ~ 12 (move), under rows by ~ 6 (stay), stairs rows by ~ 5 (stay) and then ~ 16 (move)."""
    assert Nk >= 192
    g = torch.Generator().manual_seed(seed)
    nb = (Nk + 63) // 64
    last32 = (Nk - 1) // 32 * 32
    i = torch.arange(Nq)
    cls = i % 20
    r = torch.randint(0, 1 << 30, (3, Nq), generator=g)
    late, under, stairs = cls < 7, (cls >= 7) & (cls < 12), (cls >= 12) & (cls < 17)
    j1 = r[0] % Nk                                                      # plain
    j1 = torch.where(late, last32 + r[0] % (Nk - last32), j1)
    j1 = torch.where(under, 64 + r[0] % (Nk - 64), j1)
    b1 = 1 + r[1] % (nb - 2)                                            # stairs: 64-key block 1 .. nb - 2
    j1 = torch.where(stairs, b1 * 64 + r[0] % 64, j1)
    lo2 = (b1 + 1) * 64
    j2 = lo2 + r[2] % (Nk - lo2).clamp_min(1)
    a1 = torch.full((Nq,), RESCALE_GAINS["plain"])
    a1[under] = RESCALE_GAINS["under"]
    a1[stairs] = RESCALE_GAINS["stairs"][0]
    a2 = torch.where(stairs, torch.tensor(RESCALE_GAINS["stairs"][1]), torch.tensor(0.0))
    q, k, v, do = _draw(seed, B, H, Nq, Nk, lambda ks: a1[:, None] * ks[j1] + a2[:, None] * ks[j2])
    pi = torch.where(stairs, j2, j1)
    return Fixture("rescale", q.to(dtype), k.to(dtype), v.to(dtype), do.to(dtype), pi, None)


# ------------------------------------------------------------------------------------------------ references
def _causal_mask(s):
    n = s.shape[-1]
    return s.masked_fill(torch.ones(s.shape[-2], n, dtype=torch.bool, device=s.device).triu(1), float("-inf"))


def _plain_slice(q, k, v, do, causal, dt):
    """softmax(q k^T / 8) v and its autograd backward in `dt`; lse in base 2."""
    q, k, v = (x.to(dt).clone().requires_grad_(True) for x in (q, k, v))
    s = (q @ k.T) * SCALE
    if causal:
        s = _causal_mask(s)
    lse = torch.logsumexp(s, -1)
    o = torch.exp(s - lse[:, None]) @ v
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], do.to(dt))
    return {"o": o.detach(), "lse": (lse * LOG2E).detach()[None], "dq": dq, "dk": dk, "dv": dv}


def ref_slice(q, k, v, do, causal=False):
    return _plain_slice(q, k, v, do, causal, torch.float64)


def _bf(x):
    return x.to(torch.bfloat16).float()


def twin_slice_bf16(q, k, v, do, causal=False):
    """The bf16 rounding policy (module docstring), written as plain fp32 torch on bf16-valued operands."""
    q, k, v, do = (x.float() for x in (q, k, v, do))
    s2 = (q @ k.T) * (SCALE * LOG2E)
    if causal:
        s2 = _causal_mask(s2)
    m = s2.amax(-1, keepdim=True)
    p = _bf(torch.exp2(s2 - m))                                     # unnormalised, rounded once
    l = p.sum(-1, keepdim=True)
    o = _bf((p @ v) / l)
    lse = m + torch.log2(l)
    pn = torch.exp2(s2 - lse)                                       # the backward recomputes P from the saved LSE
    dv = _bf(_bf(pn).T @ do)
    delta = (do * o).sum(-1, keepdim=True)
    ds = _bf(pn * (do @ v.T - delta))
    return {"o": o, "lse": lse[:, 0][None], "dq": _bf((ds @ k) * SCALE), "dk": _bf((ds.T @ q) * SCALE), "dv": dv}


def yard_slice(q, k, v, do, causal, dtype):
    if dtype == torch.float32:
        return _plain_slice(q, k, v, do, causal, torch.float32)
    return twin_slice_bf16(q, k, v, do, causal)


def _stack(fx, fn, device):
    out = {t: [] for t in TENSORS}
    for b in range(fx.B):
        for h in range(fx.H):
            r = fn(*fx.slice(b, h, device))
            for t in TENSORS:
                out[t].append(r[t])
    # o / dq: [B*H, Nq, 64]; dk / dv: [B*H, Nk, 64]; lse: [B*H, 1, Nq] (one "row" per slice)
    return {t: torch.stack(out[t]) for t in TENSORS}


def reference(fx, device="cpu"):
    """fp64 o, lse (base 2), dq, dk, dv, one (b, h) slice at a time on `device`."""
    return _stack(fx, lambda q, k, v, do: ref_slice(q, k, v, do, fx.causal), device)


def yardstick(fx, device="cpu"):
    return _stack(fx, lambda q, k, v, do: yard_slice(q, k, v, do, fx.causal, fx.dtype), device)


def check_reference_slice(fx, ref, b, h):
    """The device reference of slice (b, h) against the same fp64 computation on the CPU: 1e-12 relative (max-norm), so that the
    reference does not depend on the GPU's BLAS."""
    cpu = ref_slice(*fx.slice(b, h), fx.causal)
    worst = 0.0
    for t in TENSORS:
        dev_t = ref[t][b * fx.H + h].cpu()
        worst = max(worst, ((dev_t - cpu[t]).abs().max() / cpu[t].abs().max()).item())
    assert worst <= 1e-12, f"device fp64 reference differs from the CPU's by {worst:.2e} (slice {b},{h})"
    return worst


# ------------------------------------------------------------------------------------------------ statistics and bound
def error_stats(got, ref, rows=None):
    """got, ref: [S, R, C].  max: global max-norm error over max |ref|; l2: relative L2; row: the worst row's max error over
    that row's max |ref|.  rows: optional bool [S, R] (or [S, C] for lse, whose "row" is the slice) restricting the elements."""
    ref = ref.double()
    e = (got.double() - ref).abs()
    if rows is not None:
        sel = rows.to(e.device)
        sel = sel[:, None, :] if e.shape[1] == 1 else sel[:, :, None]
        e, ref = e * sel, ref * sel
    rmax = ref.abs().amax(-1)
    row = torch.where(rmax > 0, e.amax(-1) / rmax.clamp_min(1e-300), torch.zeros_like(rmax))
    return {"max": (e.max() / ref.abs().max()).item(), "l2": (e.norm() / ref.norm()).item(), "row": row.max().item(),
            "worst_row": int(row.flatten().argmax())}


def ulp(dtype, x):
    return 2.0 ** (math.floor(math.log2(x)) - {torch.bfloat16: 7, torch.float32: 23}[dtype])


def floor_rel(name, ref, dtype):
    """The floor of the bound, relative to the tensor's maximum: 8 ulp of the compute dtype at that maximum.  lse is stored in fp32
    whatever the compute dtype, so 8 bf16 ulp of its own value (0.5 at |lse| ~ 12) would bound nothing; its floor comes from what
    it is computed from instead: lse = m + log2(sum P) with every P rounded to the compute dtype once, so one ulp of a
    probability (2^-7 relative in bf16, twice the worst rounding) moves it by log2(e) * 2^-7 - and never less than 8 fp32 ulp."""
    mx = ref.abs().max().item()
    if name == "lse":
        return max(8.0 * ulp(torch.float32, mx), LOG2E * ulp(dtype, 1.0)) / mx
    return 8.0 * ulp(dtype, mx) / mx


def bounds(name, ref, yard, dtype, rows=None):
    ys = error_stats(yard, ref, rows)
    fl = floor_rel(name, ref, dtype)
    return {s: max(FACTOR * ys[s], fl) for s in STATS}, ys


def compare(name, got, ref, yard, dtype, rows=None):
    """(ok, line, ratios): every statistic of got-vs-ref within its bound; ratios = kernel error / yardstick error."""
    bd, ys = bounds(name, ref, yard, dtype, rows)
    gs = error_stats(got, ref, rows)
    finite = bool(torch.isfinite(got.float()).all())
    ok = finite and all(gs[s] <= bd[s] for s in STATS)
    ratios = {s: gs[s] / max(ys[s], 1e-300) for s in STATS}
    line = f"{name:3s} " + " ".join(f"{s}: {gs[s]:.2e} / yard {ys[s]:.2e} = {ratios[s]:.2f} (bound {bd[s]:.2e})" for s in STATS)
    if not ok:
        line += f"  FAIL worst row {gs['worst_row']}" + ("" if finite else " non-finite")
    return ok, line, ratios


# ------------------------------------------------------------------------------------------------ fixture conditions
def scores2(fx, b, h, device="cpu"):
    """fp64 scaled scores in base 2 of one slice."""
    q, k, _, _ = fx.slice(b, h, device)
    s = (q.double() @ k.double().T) * (SCALE * LOG2E)
    return _causal_mask(s) if fx.causal else s


def pmax_median(fx, device="cpu"):
    """Median over all rows of the row-maximum probability (fp64)."""
    pm = []
    for b in range(fx.B):
        for h in range(fx.H):
            pm.append(torch.softmax(scores2(fx, b, h, device) / LOG2E, -1).amax(-1))
    return torch.cat(pm).median().item()


def rescale_rows(fx, kvb, device="cpu"):
    """Walks key blocks of `kvb` over the fp64 scores the way the forward's lazy reference does: the reference starts at the
    first block's maximum and moves to a later block's maximum only when that exceeds it by more than 8.  Returns bool
    [B*H, Nq] masks (moved: the reference moved after the first block; under: some later block exceeded the current
    reference by 4..8 and it stayed)."""
    moved, under = [], []
    for b in range(fx.B):
        for h in range(fx.H):
            s = scores2(fx, b, h, device)
            m = s[:, :kvb].amax(-1)
            mv = torch.zeros_like(m, dtype=torch.bool)
            un = torch.zeros_like(mv)
            for k0 in range(kvb, fx.Nk, kvb):
                mx = s[:, k0:k0 + kvb].amax(-1)
                go = mx > m + 8.0
                un |= ~go & (mx > m + 4.0)
                mv |= go
                m = torch.where(go, mx, m)
            moved.append(mv)
            under.append(un)
    return torch.stack(moved), torch.stack(under)


# ------------------------------------------------------------------------------------------------ mutations of the reference
def _sub(fx, q=None, k=None, v=None, do=None):
    return Fixture(fx.kind, fx.q if q is None else q, fx.k if k is None else k, fx.v if v is None else v,
                   fx.do if do is None else do, fx.pi, fx.gain, fx.causal)


def mutate_delete_last_key(fx, device="cpu"):
    """What a kernel that never reads the last key would compute (dk / dv of the surviving keys)."""
    r = reference(_sub(fx, k=fx.k[:, :, :-1], v=fx.v[:, :, :-1]), device)
    return r, {"o": slice(None), "lse": slice(None), "dq": slice(None), "dk": slice(0, fx.Nk - 1), "dv": slice(0, fx.Nk - 1)}


def mutate_delete_last_query(fx, device="cpu"):
    """What a kernel that never reads the last query would compute (o / dq of the surviving queries)."""
    r = reference(_sub(fx, q=fx.q[:, :, :-1], do=fx.do[:, :, :-1]), device)
    nq = slice(0, fx.Nq - 1)
    return r, {"o": nq, "lse": nq, "dq": nq, "dk": slice(None), "dv": slice(None)}


def swap_pair(fx):
    """A planted key and its neighbour in the same 16-row tile."""
    for r0 in fx.pi.tolist():
        if r0 >= 0 and (r0 ^ 1) < fx.Nk:
            return r0, r0 ^ 1
    raise AssertionError("no planted key with a neighbour")


def mutate_swap_v_rows(fx, r0, r1, device="cpu"):
    """What a kernel that exchanges two V rows of one 16-row tile would compute."""
    assert r0 // 16 == r1 // 16 and r0 != r1
    v = fx.v.clone()
    v[:, :, r0], v[:, :, r1] = fx.v[:, :, r1], fx.v[:, :, r0]
    return reference(_sub(fx, v=v), device), {t: slice(None) for t in TENSORS}


def mutation_effect(name, ref, mut, keep):
    """error_stats of the mutated reference against the true one, on the rows both have."""
    if name == "lse":
        return error_stats(mut[name], ref[name][:, :, keep])
    return error_stats(mut[name], ref[name][:, keep])


# ------------------------------------------------------------------------------------------------ the cases both test files use
# (B, H, Nq, Nk, dtype, forward form, dQ form, dK/dV form, nsplit): what the library's own dispatch must choose
PRODUCTION_CASES = [
    (8, 5, 4096, 4096, "bf16", 2, 2, 2, 1),
    (8, 5, 4096, 4096, "f32", 2, 1, 1, 1),
    (8, 10, 1024, 1024, "bf16", 2, 2, 2, 1),
    (16, 20, 256, 256, "bf16", 2, 2, 2, 1),         # exactly at Nk >= 256 (and 2 * 20 * 16 = 640 >= 384)
    (8, 20, 256, 256, "bf16", 1, 1, 1, 1),          # 2 * 20 * 8 = 320: just under 384
    (8, 5, 4096, 77, "bf16", 1, 1, 1, 4),           # cross-attention, dK/dV splits the query sweep
    (8, 10, 1024, 77, "bf16", 1, 1, 1, 1),          # 2 * 10 * 8 = 160 key-block workgroups: no split
]
RAGGED_N = (65, 128, 129, 192, 193, 300, 333)
RAGGED_CROSS = ((200, 77), (256, 13))
RESCALE_NK = (256, 300, 4096)
RESCALE_SEED = 11
CAUSAL_N = (77, 130)
CLAMP_SHAPE = (1, 2, 4096, 77)

# Seeds chosen so that the fp64 reference ALONE meets the sensitivity conditions of tests/test_attention_host.py (whether the
# query planted on the last key, or the last query, carries a large enough gradient row is a matter of the draw).
SEEDS = {(192, 192, "mid"): 3, (256, 256, "mid"): 3, (300, 300, "mid"): 3, (4096, 77, "peaked"): 3, (4096, 77, "mid"): 7}   # others: 1


def seed_for(Nq, Nk, regime):
    return SEEDS.get((Nq, Nk, regime), 1)


def causal_seed(N):
    return SEEDS.get((N, N, "causal"), 1)


CLAMP_SEED = seed_for(4096, 77, "mid")
