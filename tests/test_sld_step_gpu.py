"""pdmk_sld_guidance, pdmk_sld_plms_step and pdmk_sld_ddim_step (csrc/sampler.hip): bit-identical to Safe Latent Diffusion's
guidance chain written in torch fp32 operations, followed by the eager chain of tests/test_plms_step_gpu.py (scheduler step,
tripled latent copy, nchw_to_nhwc).

The oracle holds every scalar as an fp32 0-dim tensor rounded from the double (`1 - mom_beta` formed in double first), so each
line below is one fp32 operation rounded once - the arithmetic contract of include/pdmk.h pdmk_sld_params.

Inputs: the safety prediction is s = t - delta with delta drawn per element from DELTAS, and t spread over several binades
(bf16 storage keeps a small delta only beside a small t), so that for the Medium preset each branch of `scale` - masked to
zero, clamped to one, strictly between - holds at least 10 % of the elements; `test_inputs_cover_the_three_branches` checks
that on the host and the GPU tests assert it again on what they feed the kernels."""
import pytest
import torch

B, C, H, W, G = 2, 4, 8, 12, 7.5
DELTAS = (-2.0, -1e-2, -1e-4, -0.0, 0.0, 1e-5, 5e-4, 0.00999, 0.01, 0.0101, 0.03, 1.0, 2.0)
PRESETS = {"Weak": (200, 15, 0.0, 0.0, 0.0), "Medium": (1000, 10, 0.01, 0.3, 0.4), "Strong": (2000, 7, 0.025, 0.5, 0.7),
           "Max": (5000, 0, 1.0, 0.5, 0.7), "never": (1500, 100, 0.02, 0.25, 0.9)}     # (scale, warm-up, threshold, mom, beta)
STEPS = (1, 2, 3, 12)


def _pred(gen, rows_per_third, ld, dtype):
    """One U-Net output [3 * rows, ld] in dtype (thirds: uncond, text, safety = text - delta), drawn on the host."""
    u = torch.randn(rows_per_third, ld, generator=gen) * 2
    binade = torch.tensor([1.0, 2.0 ** -8, 2.0 ** -10, 2.0 ** -12])[torch.randint(0, 4, (rows_per_third, ld), generator=gen)]
    t = (torch.randn(rows_per_third, ld, generator=gen) * 2 * binade).to(dtype)
    delta = torch.tensor(DELTAS)[torch.randint(0, len(DELTAS), (rows_per_third, ld), generator=gen)]
    s = (t.float() - delta).to(dtype)
    return torch.cat([u.to(dtype), t, s])


def _branch_shares(pred, scale, threshold):
    """Shares of the elements whose `scale` is masked to zero, clamped to one, strictly between 0 and 1 (fp32 arithmetic)."""
    n = pred.shape[0] // 3
    t, s = pred[n:2 * n].float(), pred[2 * n:].float()
    d = t - s
    raw = d.abs() * torch.tensor(scale, dtype=torch.float32)
    masked = d >= torch.tensor(threshold, dtype=torch.float32)
    clamped = ~masked & (raw >= 1)
    between = ~masked & (raw > 0) & (raw < 1)
    return [float(x.float().mean()) for x in (masked, clamped, between)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inputs_cover_the_three_branches(dtype):
    gen = torch.Generator().manual_seed(0)
    pred = _pred(gen, B * H * W, 16, dtype)
    shares = _branch_shares(pred[:, :C], PRESETS["Medium"][0], PRESETS["Medium"][2])
    print(dtype, "masked / clamped / between:", shares)
    assert min(shares) >= 0.10, shares


class _Oracle:
    """The chain of the issue in torch fp32 operations; the momentum lives here."""

    def __init__(self, preset, g, shape, dev):
        scale, self.warmup, thr, mom, beta = preset
        f = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)
        self.scale, self.thr, self.mom_scale, self.beta, self.omb, self.g = f(scale), f(thr), f(mom), f(beta), f(1.0 - beta), f(g)
        self.m = torch.zeros(shape, device=dev)

    def __call__(self, u, t, s, i):
        d = t - s
        scale = torch.clamp(d.abs() * self.scale, max=1.0)
        scale = torch.where(d >= self.thr, torch.zeros_like(scale), scale)
        gs = (s - u) * scale
        gs = gs + self.mom_scale * self.m
        self.m = self.beta * self.m + self.omb * gs
        ng = t - u
        if i >= self.warmup:
            ng = ng - gs
        return u + self.g * ng


def _scheduler(kind, prediction_type, steps):
    from pdm.pipelines.pruning_pipelines import DDIMScheduler, PNDMScheduler
    sch = (PNDMScheduler if kind == "plms" else DDIMScheduler)(prediction_type=prediction_type)
    sch.set_timesteps(steps)
    return sch


def _run(dev, kind, dtype, prediction_type, steps, preset, check=True):
    """All U-Net calls of one schedule through the fused SLD step, checked against the oracle after every call.  Returns what
    the kernel left after each call."""
    from pdm import _pdmk as k
    from pdm.models.unet.spec import padc
    cp, ld = padc(C), padc(C) + 8
    HW, n = H * W, B * C * H * W
    gen = torch.Generator().manual_seed(steps)
    sch = _scheduler(kind, prediction_type, steps)
    rows = sch.plms_rows() if kind == "plms" else sch.ddim_rows()
    N = len(rows)
    table = (k.plms_table if kind == "plms" else k.ddim_table)(rows, dev)
    params = k.sld_params(*preset)
    oracle = _Oracle(preset, G, (B, C, H, W), dev)
    lat = torch.randn(B, C, H, W, generator=gen).to(dev)
    sample, mom = lat.reshape(-1).clone(), torch.zeros(n, device=dev)
    cur, ets = torch.zeros(n, device=dev), torch.zeros(4, n, device=dev)
    state = torch.zeros(2, device=dev, dtype=torch.int32)
    t_out = torch.zeros(3 * B, device=dev, dtype=torch.int64)
    x_next = torch.full((3 * B * HW, cp), 3.0, device=dev, dtype=dtype)          # padding must come back as zeros

    def launch(pred):
        if kind == "plms":
            k.sld_plms_step(pred, ld, G, params, mom, sample, cur, ets, table, N, state, t_out, x_next, cp, B, C, HW)
        else:
            k.sld_ddim_step(pred, ld, G, params, mom, sample, table, N, state, t_out, x_next, cp, B, C, HW)

    trace, appended = [], 0
    for i in range(N):
        host_pred = _pred(gen, B * HW, ld, dtype)
        if check and i == 0:
            shares = _branch_shares(host_pred[:, :C], PRESETS["Medium"][0], PRESETS["Medium"][2])
            assert min(shares) >= 0.10, shares
        pred = host_pred.to(dev)
        launch(pred)
        trace.append([x.clone() for x in (sample, x_next, mom, ets, cur, t_out, state)])
        if not check:
            continue
        what = f"{kind} {steps} steps, call {i}"
        out = torch.empty(3 * B, C, H, W, device=dev)
        k.nhwc_to_nchw(pred, out, 3 * B, C, HW, ld)
        m_before = oracle.m.clone()
        noise = oracle(out[:B], out[B:2 * B], out[2 * B:], i)
        # the eager loop's kernel on the same operands
        alone, m_alone = torch.empty(B, C, H, W, device=dev), m_before.clone()
        k.sld_guidance(out, alone, m_alone, G, params, i >= preset[1])
        assert torch.equal(alone, noise) and torch.equal(m_alone, oracle.m), what
        lat = sch.step(noise.contiguous(), int(sch.timesteps[i]), lat, return_dict=False)[0]
        x_ref = torch.empty(3 * B * HW, cp, device=dev, dtype=dtype)
        k.nchw_to_nhwc(torch.cat([lat, lat, lat]).contiguous(), x_ref, 3 * B, C, HW, cp)
        assert torch.equal(sample.view(B, C, H, W), lat), what
        assert torch.equal(x_next, x_ref), what
        assert torch.equal(mom.view(B, C, H, W), oracle.m), what
        assert state.tolist() == [i + 1, 0], what
        if i + 1 < N:
            assert t_out.tolist() == [int(sch.timesteps[i + 1])] * (3 * B), what
        if kind == "plms":
            if i != 1:
                appended += 1
            for j, e in enumerate(reversed(sch.ets)):           # history: ets[-1 - j] lives in ring slot (appended - 1 - j) % 4
                assert torch.equal(ets[(appended - 1 - j) % 4].view(B, C, H, W), e), (what, j)
            if sch.cur_sample is not None:
                assert torch.equal(cur.view(B, C, H, W), sch.cur_sample), what
    if check:                                                   # a launch past the end of the table changes nothing
        launch(pred)
        assert all(torch.equal(a, b) for a, b in zip(trace[-1], (sample, x_next, mom, ets, cur, t_out, state)))
    return trace


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_sld_step_equals_torch_chain(dev, kind, prediction_type, dtype):
    for steps in STEPS:
        for name, preset in PRESETS.items():
            _run(dev, kind, dtype, prediction_type, steps, preset)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_sld_step_two_runs_bit_equal(dev, kind):
    a = _run(dev, kind, torch.bfloat16, "v_prediction", 12, PRESETS["Medium"], check=False)
    b = _run(dev, kind, torch.bfloat16, "v_prediction", 12, PRESETS["Medium"], check=False)
    assert len(a) == len(b) == (13 if kind == "plms" else 12)
    assert all(torch.equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 4, 8, 12), (1, 3, 5, 7), (3, 4, 17, 16)])
@pytest.mark.parametrize("offset", [0, 1])
def test_sld_guidance_equals_torch_chain(dev, shape, offset):
    """Both access widths of pdmk_sld_guidance (n % 4 != 0 or an unaligned momentum take the scalar one), both sides of the
    warm-up, every preset, three consecutive calls so that the momentum feeds back."""
    from pdm import _pdmk as k
    b, c, h, w = shape
    n = b * c * h * w
    gen = torch.Generator().manual_seed(n + offset)
    for name, preset in PRESETS.items():
        params = k.sld_params(*preset)
        oracle = _Oracle(preset, G, shape, dev)
        mom = torch.zeros(n + offset, device=dev)[offset:].view(shape)
        for i in (0, preset[1], preset[1] + 1):
            pred = _pred(gen, n, 1, torch.float32).view(3 * b, c, h, w).to(dev)
            want = oracle(pred[:b], pred[b:2 * b], pred[2 * b:], i)
            got = torch.empty(shape, device=dev)
            k.sld_guidance(pred, got, mom, G, params, i >= preset[1])
            assert torch.equal(got, want) and torch.equal(mom, oracle.m), (name, i)
