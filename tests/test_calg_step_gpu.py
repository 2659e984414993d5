"""pdmk_calg_dots, pdmk_calg_guidance, pdmk_calg_plms_step and pdmk_calg_ddim_step (csrc/sampler.hip; include/pdmk.h "Concept
algebra"), in the manner of tests/test_sld_step_gpu.py.

Scalars.  nrm = (float)sqrt(S_dd) and dot = (float)(S_wd / sqrt(S_dd)) read back from `scalars` are compared with a torch fp64
evaluation of the same sums; the bound is 4 x d_ref, d_ref the relative distance of the reference's own fp32 torch chain
(`sqrt((u ** 2).sum())`, `(noise_tmp * u).sum()`) from that fp64 evaluation on the same inputs, measured on the host and
printed.  A correct kernel always passes: it returns the fp32 number nearest to the fp64 value, and the reference's result is
an fp32 number too, so d_ref is never below the kernel's distance (beyond fp64 summation noise of 1e-16).

Elements.  Given the kernel's own two scalars, every output must be bit-equal to the seven-operation fp32 chain
    d = p1 - p0;  e = d / nrm;  pw = dot * e;  t2 = t - pw;  ng = t2 - u;  gn = g * ng;  out = u + gn
followed by the scheduler's step and nchw_to_nhwc of the five copies.  The chain is evaluated on the host (IEEE fp32, each
operation rounded once), the scheduler step on the device as in the other step tests.  The step kernels repeat the arithmetic
of pdmk_axpby's 16-byte path (csrc/sampler.hip, header); pdmk_axpby itself leaves the last n % 4 elements to a scalar tail that
the compiler contracts differently, so for the shape with n % 4 != 0 the oracle's scheduler runs on the latents padded with
zeros to a multiple of four and every element goes through the path the kernels reproduce.

Inputs: five fifths drawn on the host, each randn * 2 in the storage dtype, and p2 = t - 0.3 (p1 - p0) + 0.1 randn, so the dot
product is signal (0.3 |d|) and not noise.  Condition, asserted on the host recipe and again on what the GPU gets: the
projection term max |dot * e| is at least 1000 ulps of the largest output (1000 x 2^-23 max |out|; the output bound itself is
bit equality) - a kernel that skips the projection cannot pass."""
import pytest
import torch

G = 7.5
STEPS = (1, 2, 3, 12)
# (B, C, H, W), extra row stride: padded rows | odd sizes, n % 4 != 0 | several partial workgroups | the 256-workgroup cap with
# more than one element per thread (72000 elements, 65536 threads)
SHAPES = [((2, 4, 8, 12), 8), ((1, 3, 5, 7), 0), ((3, 4, 17, 16), 0), ((5, 4, 60, 60), 0)]
IDS = ["2x4x8x12+ld", "1x3x5x7", "3x4x17x16", "5x4x60x60"]


def _pred(gen, rows, ld, dtype):
    """One U-Net output [5 * rows, ld] in dtype (fifths: u, t, p0, p1, p2), drawn on the host."""
    u, t, p0, p1 = ((torch.randn(rows, ld, generator=gen) * 2).to(dtype) for _ in range(4))
    p2 = (t.float() - 0.3 * (p1.float() - p0.float()) + 0.1 * torch.randn(rows, ld, generator=gen)).to(dtype)
    return torch.cat([u, t, p0, p1, p2])


def _nchw(pred, R, C, H, W):
    """Host rows [R * H * W, ld] -> fp32 NCHW [R, C, H, W] (exact)."""
    return pred[:, :C].float().reshape(R, H * W, C).permute(0, 2, 1).reshape(R, C, H, W).contiguous()


def _sums64(out5, B):
    """(nrm, dot) in fp64 from fp32 differences, as the contract states them."""
    t, p0, p1, p2 = (out5[j * B:(j + 1) * B] for j in range(1, 5))
    d, w = (p1 - p0).double(), (t - p2).double()
    nrm = (d * d).sum().sqrt()
    return nrm, (w * d).sum() / nrm


def _reference32(out5, B):
    """(nrm, dot) of the reference's own fp32 chain (concept_algebra.py:113-118)."""
    t, p0, p1, p2 = (out5[j * B:(j + 1) * B].clone() for j in range(1, 5))
    tmp = t - p2
    u = p1 - p0
    nrm = torch.sqrt((u ** 2).sum())
    u /= nrm
    return nrm, (tmp * u).sum()


def _chain(out5, B, nrm, dot):
    """The seven fp32 operations on the host; nrm, dot fp32 0-dim tensors.  Returns (guided noise, projection term)."""
    u, t, p0, p1 = (out5[j * B:(j + 1) * B] for j in range(4))
    g = torch.tensor(G, dtype=torch.float32)
    if float(nrm) > 0:
        d = p1 - p0
        e = d / nrm
        pw = dot * e
    else:
        pw = torch.zeros_like(t)
    t2 = t - pw
    ng = t2 - u
    gn = g * ng
    return u + gn, pw


def _condition(noise, pw):
    return float(pw.abs().max()), 1000 * 2.0 ** -23 * float(noise.abs().max())


def host_condition(shape, extra, dtype):
    """The recipe's condition on the host, with the scalars of the fp64 evaluation (tests/test_debias_sampling_host.py)."""
    B, C, H, W = shape
    pred = _pred(torch.Generator().manual_seed(0), B * H * W, C + extra, dtype)
    out5 = _nchw(pred, 5 * B, C, H, W)
    nrm, dot = _sums64(out5, B)
    return _condition(*_chain(out5, B, nrm.float(), dot.float()))


def _scheduler(kind, prediction_type, steps):
    from pdm.pipelines.pruning_pipelines import DDIMScheduler, PNDMScheduler
    sch = (PNDMScheduler if kind == "plms" else DDIMScheduler)(prediction_type=prediction_type)
    sch.set_timesteps(steps)
    return sch


def _run(dev, kind, dtype, prediction_type, steps, shape, extra, check=True, degenerate=False):
    """All U-Net calls of one schedule through calg_dots + the fused step, checked against the oracle after every call.
    Returns what the kernels left after each call (partial workspace and scalars included)."""
    from pdm import _pdmk as k
    from pdm.models.unet.spec import padc
    B, C, H, W = shape
    cp, ld = padc(C), padc(C) + extra
    HW, n = H * W, B * C * H * W
    gen = torch.Generator().manual_seed(steps)
    sch = _scheduler(kind, prediction_type, steps)
    rows = sch.plms_rows() if kind == "plms" else sch.ddim_rows()
    N = len(rows)
    table = (k.plms_table if kind == "plms" else k.ddim_table)(rows, dev)
    lat = torch.randn(B, C, H, W, generator=gen).to(dev)
    sample = lat.reshape(-1).clone()
    pad = lambda x: torch.nn.functional.pad(x.reshape(-1), (0, -n % 4)).view(1, 1, 1, -1)      # the oracle's scheduler buffers
    unpad = lambda x: x.reshape(-1)[:n].view(B, C, H, W)
    lat_p = pad(lat)
    cur, ets = torch.zeros(n, device=dev), torch.zeros(4, n, device=dev)
    state = torch.zeros(2, device=dev, dtype=torch.int32)
    t_out = torch.zeros(5 * B, device=dev, dtype=torch.int64)
    x_next = torch.full((5 * B * HW, cp), 3.0, device=dev, dtype=dtype)          # padding must come back as zeros
    nws = k.calg_workspace_elems(B, C, HW)
    assert nws == 2 * min(256, -(-n // 256))
    ws = torch.full((nws,), -1.0, device=dev, dtype=torch.float64)
    scalars = torch.full((2,), -1.0, device=dev)

    def launch(pred):
        k.calg_dots(pred, ld, B, C, HW, ws)
        if kind == "plms":
            k.calg_plms_step(pred, ld, G, ws, scalars, sample, cur, ets, table, N, state, t_out, x_next, cp, B, C, HW)
        else:
            k.calg_ddim_step(pred, ld, G, ws, scalars, sample, table, N, state, t_out, x_next, cp, B, C, HW)

    trace, appended = [], 0
    for i in range(N):
        host_pred = _pred(gen, B * HW, ld, dtype)
        if degenerate:
            host_pred[3 * B * HW:4 * B * HW] = host_pred[2 * B * HW:3 * B * HW]
        pred = host_pred.to(dev)
        launch(pred)
        trace.append([x.clone() for x in (sample, x_next, ets, cur, t_out, state, ws, scalars)])
        if not check:
            continue
        what = f"{kind} {steps} steps, call {i}"
        out5 = _nchw(host_pred, 5 * B, C, H, W)
        nrm, dot = scalars.cpu()
        noise, pw = _chain(out5, B, nrm, dot)
        if degenerate:
            assert scalars.tolist() == [0.0, 0.0] and torch.isfinite(noise).all(), what
        else:
            have, need = _condition(noise, pw)
            assert have >= need, (what, have, need)
        noise = noise.to(dev)
        # the eager loop's two launches on the same operands, fp32 NCHW: the same partial sums, scalars and elements
        out_dev = out5.to(dev)
        ws_e, sc_e = torch.zeros_like(ws), torch.zeros_like(scalars)
        alone = torch.empty(B, C, H, W, device=dev)
        k.calg_dots(out_dev, 1, B, 1, C * HW, ws_e)
        k.calg_guidance(out_dev, alone, G, ws_e, sc_e)
        assert torch.equal(ws_e, ws) and torch.equal(sc_e, scalars) and torch.equal(alone, noise), what
        lat_p = sch.step(pad(noise), int(sch.timesteps[i]), lat_p, return_dict=False)[0]
        lat = unpad(lat_p)
        x_ref = torch.empty(5 * B * HW, cp, device=dev, dtype=dtype)
        k.nchw_to_nhwc(torch.cat([lat] * 5).contiguous(), x_ref, 5 * B, C, HW, cp)
        assert torch.equal(sample.view(B, C, H, W), lat), what
        assert torch.equal(x_next, x_ref), what
        assert state.tolist() == [i + 1, 0], what
        if i + 1 < N:
            assert t_out.tolist() == [int(sch.timesteps[i + 1])] * (5 * B), what
        if kind == "plms":
            if i != 1:
                appended += 1
            for j, e in enumerate(reversed(sch.ets)):           # history: ets[-1 - j] lives in ring slot (appended - 1 - j) % 4
                assert torch.equal(ets[(appended - 1 - j) % 4].view(B, C, H, W), unpad(e)), (what, j)
            if sch.cur_sample is not None:
                assert torch.equal(cur.view(B, C, H, W), unpad(sch.cur_sample)), what
    if check:                                                   # a launch past the end of the table changes nothing
        before = [x.clone() for x in (sample, x_next, ets, cur, t_out, state, scalars)]
        if kind == "plms":
            k.calg_plms_step(pred, ld, G, ws, scalars, sample, cur, ets, table, N, state, t_out, x_next, cp, B, C, HW)
        else:
            k.calg_ddim_step(pred, ld, G, ws, scalars, sample, table, N, state, t_out, x_next, cp, B, C, HW)
        assert all(torch.equal(a, b) for a, b in zip(before, (sample, x_next, ets, cur, t_out, state, scalars)))
    return trace


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,extra", SHAPES, ids=IDS)
def test_calg_scalars_against_fp64(dev, shape, extra, dtype):
    from pdm import _pdmk as k
    from pdm.models.unet.spec import padc
    B, C, H, W = shape
    ld, HW = padc(C) + extra, H * W
    host_pred = _pred(torch.Generator().manual_seed(B * C * HW), B * HW, ld, dtype)
    out5 = _nchw(host_pred, 5 * B, C, H, W)
    want = _sums64(out5, B)
    d_ref = [abs(float(r) - float(w)) / abs(float(w)) for r, w in zip(_reference32(out5, B), want)]
    pred = host_pred.to(dev)
    ws = torch.zeros(k.calg_workspace_elems(B, C, HW), device=dev, dtype=torch.float64)
    scalars, out = torch.zeros(2, device=dev), torch.empty(B, C, H, W, device=dev)
    k.calg_dots(pred, ld, B, C, HW, ws)
    assert ws.numel() <= 512
    # the pairs themselves: sums of squares are positive, and their totals are the fp64 sums
    pairs = ws.view(-1, 2).cpu()
    assert (pairs[:, 0] > 0).all()
    assert abs(float(pairs[:, 0].sum().sqrt()) - float(want[0])) <= 1e-12 * float(want[0])
    k.calg_guidance(out5.to(dev), out, G, ws, scalars)
    got = scalars.cpu()
    for name, g, w, dr in zip(("nrm", "dot"), got, want, d_ref):
        dist = abs(float(g) - float(w)) / abs(float(w))
        print(f"{shape} {dtype} {name}: d_ref {dr:.3e}  kernel {dist:.3e}")
        assert dist <= 4 * dr, (name, dist, dr)
    have, need = _condition(*_chain(out5, B, got[0], got[1]))
    assert have >= need, (have, need)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("kind", ["plms", "ddim"])
@pytest.mark.parametrize("shape,extra", SHAPES, ids=IDS)
def test_calg_step_equals_torch_chain(dev, shape, extra, kind, prediction_type, dtype):
    for steps in STEPS:
        _run(dev, kind, dtype, prediction_type, steps, shape, extra)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_calg_equal_concepts_leave_the_projection_out(dev, kind):
    """p1 == p0: S_dd = 0, where the reference divides by zero.  The scalars come back as (0, 0) and the chain runs with a zero
    projection term: plain guidance, no NaN."""
    _run(dev, kind, torch.bfloat16, "v_prediction", 3, *SHAPES[0], degenerate=True)
    _run(dev, kind, torch.float32, "epsilon", 2, *SHAPES[1], degenerate=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_calg_step_two_runs_bit_equal(dev, kind):
    a = _run(dev, kind, torch.bfloat16, "v_prediction", 12, *SHAPES[3], check=False)
    b = _run(dev, kind, torch.bfloat16, "v_prediction", 12, *SHAPES[3], check=False)
    assert len(a) == len(b) == (13 if kind == "plms" else 12)
    assert all(torch.equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 4, 8, 12), (1, 3, 5, 7), (3, 4, 17, 16), (1, 1, 1, 1)])
@pytest.mark.parametrize("offset", [0, 1])
def test_calg_guidance_access_forms(dev, shape, offset):
    """Both access widths of pdmk_calg_guidance: n % 4 != 0 ((1, 3, 5, 7): 105, (1, 1, 1, 1)) or an output that is not 16-byte
    aligned (offset 1) take the scalar one.  The elements around the output stay untouched."""
    from pdm import _pdmk as k
    b, c, h, w = shape
    n = b * c * h * w
    out5 = _nchw(_pred(torch.Generator().manual_seed(n + offset), n, 1, torch.float32), 5 * b, 1, c * h, w).view(5 * b, c, h, w)
    ws = torch.zeros(k.calg_workspace_elems(b, c, h * w), device=dev, dtype=torch.float64)
    scalars = torch.zeros(2, device=dev)
    buf = torch.full((n + offset + 3,), 9.0, device=dev)
    got = buf[offset:offset + n].view(shape)
    pred = out5.to(dev)
    k.calg_dots(pred, 1, b, 1, c * h * w, ws)
    k.calg_guidance(pred, got, G, ws, scalars)
    nrm, dot = scalars.cpu()
    want, pw = _chain(out5, b, nrm, dot)
    assert torch.equal(got.cpu(), want)
    assert (buf[:offset] == 9.0).all() and (buf[offset + n:] == 9.0).all()
    assert float(pw.abs().max()) > 0
