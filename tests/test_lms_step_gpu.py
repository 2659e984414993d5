"""K-LMS on the GPU (-m gpu): pdmk_lms_step / pdmk_sld_lms_step / pdmk_calg_lms_step (csrc/sampler.hip) bit-identical to the
eager chains they replace, pdmk_timestep_embed_f32 against the int64 entry and the torch formula, the eager fp32 step against the
restatement of diffusers' scheduler in tests/lms_fixtures.py, the captured loop against the eager loop on a tiny pipeline, and
generate_images.py --scheduler lms end to end."""
import csv
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lms_fixtures as LF  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, H, W, G = 2, 4, 8, 12, 7.5
STEPS = (1, 2, 3, 5, 10)          # every order, the ring wrap (step 4 writes slot 0 again) and the last row


def _sched(prediction_type, steps):
    from pdm.pipelines.pruning_pipelines import LMSDiscreteScheduler
    sch = LMSDiscreteScheduler(prediction_type=prediction_type)
    sch.set_timesteps(steps)
    return sch


def _tail(sch, i, lat, noise, R, dtype, cp):
    """The eager loop from the guided prediction on: LMSDiscreteScheduler.step, then the next call's R / B latent copies,
    scale_model_input at the next timestep and nchw_to_nhwc.  Returns (new latents, next U-Net input)."""
    from pdm import _pdmk as k
    lat = sch.step(noise.contiguous(), sch.timesteps[i].item(), lat, return_dict=False)[0]
    x2 = torch.cat([lat] * (R // B)).contiguous()
    if i + 1 < len(sch.timesteps):
        x2 = sch.scale_model_input(x2, sch.timesteps[i + 1].item())
    x = torch.empty(R * H * W, cp, device=lat.device, dtype=dtype)
    k.nchw_to_nhwc(x2, x, R, C, H * W, cp)
    return lat, x


def _check_state(sch, i, N, R, sample, lat, x_next, x_ref, hist, state, t_out, what):
    assert torch.equal(sample.view(B, C, H, W), lat), what
    assert torch.equal(x_next, x_ref), what
    assert not x_next[:, C:].any(), what                                # padding channels zero
    assert state.tolist() == [i + 1, 0], what
    if i + 1 < N:
        assert t_out.dtype == torch.float32 and t_out.tolist() == [sch.timesteps[i + 1].item()] * R, what
    for j, d in enumerate(reversed(sch.derivatives)):                   # the derivative of step i - j lives in slot (i - j) % 4
        assert torch.equal(hist[(i - j) % 4].view(B, C, H, W), d), (what, j)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_lms_step_equals_eager_chain(dev, dtype, cfg, prediction_type):
    from pdm import _pdmk as k
    from pdm.models.unet.spec import padc
    cp, ld = padc(C), padc(C) + 8                     # the prediction's row stride differs from the input's
    R = 2 * B if cfg else B
    n = B * C * H * W
    for steps in STEPS:
        gen = torch.Generator(device=dev).manual_seed(steps)
        sch = _sched(prediction_type, steps)
        rows = sch.lms_rows()
        N = len(rows)
        assert N == steps
        table = k.lms_table(rows, dev)
        lat = torch.randn(B, C, H, W, device=dev, generator=gen) * sch.init_noise_sigma
        sample, hist = lat.reshape(-1).clone(), torch.zeros(4, n, device=dev)
        state = torch.zeros(2, device=dev, dtype=torch.int32)
        t_out = torch.zeros(R, device=dev, dtype=torch.float32)
        x_next = torch.full((R * H * W, cp), 3.0, device=dev, dtype=dtype)      # padding must come back as zeros
        for i in range(N):
            pred = (torch.randn(R * H * W, ld, device=dev, generator=gen) * 2).to(dtype)
            out = torch.empty(R, C, H, W, device=dev)
            k.nhwc_to_nchw(pred, out, R, C, H * W, ld)
            noise = out
            if cfg:
                noise = out[B:]
                k.axpby(out[:B], noise, 1.0 - G, G)
            lat, x_ref = _tail(sch, i, lat, noise, R, dtype, cp)
            k.lms_step(pred, ld, 1.0 - G, G, cfg, sample, hist, table, N, state, t_out, x_next, cp, B, C, H * W)
            _check_state(sch, i, N, R, sample, lat, x_next, x_ref, hist, state, t_out, f"steps {steps}, step {i}")
        # a launch past the end of the table changes nothing
        before = [t.clone() for t in (sample, hist, x_next, state, t_out)]
        k.lms_step(pred, ld, 1.0 - G, G, cfg, sample, hist, table, N, state, t_out, x_next, cp, B, C, H * W)
        assert all(torch.equal(a, b) for a, b in zip(before, (sample, hist, x_next, state, t_out)))


def test_lms_step_refuses_bad_arguments(dev):
    from pdm import _pdmk as k
    from pdm.models.unet.spec import padc
    cp = padc(C)
    n, HW = B * C * H * W, H * W
    sch = _sched("epsilon", 3)
    table = k.lms_table(sch.lms_rows(), dev)
    pred = torch.zeros(2 * B * HW, cp, device=dev)
    sample, hist = torch.zeros(n, device=dev), torch.zeros(4, n, device=dev)
    state = torch.zeros(2, device=dev, dtype=torch.int32)
    x_next = torch.zeros(2 * B * HW, cp, device=dev)
    with pytest.raises(k.PdmkError):                  # int64 timesteps are the other schedulers'
        k.lms_step(pred, cp, 1.0 - G, G, True, sample, hist, table, 3, state, torch.zeros(2 * B, device=dev, dtype=torch.int64),
                   x_next, cp, B, C, HW)
    t_out = torch.zeros(2 * B, device=dev)
    with pytest.raises(k.PdmkError):                  # a table of another length
        k.lms_step(pred, cp, 1.0 - G, G, True, sample, hist, table, 4, state, t_out, x_next, cp, B, C, HW)
    with pytest.raises(k.PdmkError):                  # a history of fewer than 4 slots
        k.lms_step(pred, cp, 1.0 - G, G, True, sample, hist[:3], table, 3, state, t_out, x_next, cp, B, C, HW)
    st = torch.cuda.current_stream().cuda_stream
    args = [pred.data_ptr(), cp, 1.0 - G, G, 1, sample.data_ptr(), hist.data_ptr(), table.data_ptr(), 3, state.data_ptr(),
            t_out.data_ptr(), x_next.data_ptr(), cp, B, C, HW, k.dt(pred), st]
    for pos, bad in ((0, None), (5, None), (6, None), (7, None), (9, None), (10, None), (11, None), (8, 0), (16, 7)):
        a = list(args)
        a[pos] = bad
        assert k._lib.pdmk_lms_step(*a) == (-2 if pos == 16 else -1), pos
    torch.cuda.synchronize()
    assert state.tolist() == [0, 0]


def test_sld_lms_step_equals_eager_chain(dev):
    """bf16, 5 steps, the warm-up boundary (2) inside them; inputs as tests/test_sld_step_gpu.py draws them."""
    from pdm import _pdmk as k
    from pdm.models.unet.spec import padc
    import test_sld_step_gpu as sld_test
    dtype, steps, preset = torch.bfloat16, 5, (1000, 2, 0.01, 0.3, 0.4)
    cp, ld = padc(C), padc(C) + 8
    HW, n, R = H * W, B * C * H * W, 3 * B
    gen = torch.Generator().manual_seed(steps)
    sch = _sched("v_prediction", steps)
    table = k.lms_table(sch.lms_rows(), dev)
    params = k.sld_params(*preset)
    lat = (torch.randn(B, C, H, W, generator=gen) * sch.init_noise_sigma).to(dev)
    sample, mom, hist = lat.reshape(-1).clone(), torch.zeros(n, device=dev), torch.zeros(4, n, device=dev)
    mom_e = torch.zeros(B, C, H, W, device=dev)
    state = torch.zeros(2, device=dev, dtype=torch.int32)
    t_out = torch.zeros(R, device=dev, dtype=torch.float32)
    x_next = torch.full((R * HW, cp), 3.0, device=dev, dtype=dtype)
    for i in range(steps):
        pred = sld_test._pred(gen, B * HW, ld, dtype).to(dev)
        out = torch.empty(R, C, H, W, device=dev)
        k.nhwc_to_nchw(pred, out, R, C, HW, ld)
        noise = torch.empty(B, C, H, W, device=dev)
        k.sld_guidance(out, noise, mom_e, G, params, i >= preset[1])
        lat, x_ref = _tail(sch, i, lat, noise, R, dtype, cp)
        k.sld_lms_step(pred, ld, G, params, mom, sample, hist, table, steps, state, t_out, x_next, cp, B, C, HW)
        _check_state(sch, i, steps, R, sample, lat, x_next, x_ref, hist, state, t_out, f"sld step {i}")
        assert torch.equal(mom.view(B, C, H, W), mom_e), i


def test_calg_lms_step_equals_eager_chain(dev):
    """bf16, 5 steps; inputs as tests/test_calg_step_gpu.py draws them."""
    from pdm import _pdmk as k
    from pdm.models.unet.spec import padc
    import test_calg_step_gpu as calg_test
    dtype, steps = torch.bfloat16, 5
    cp, ld = padc(C), padc(C) + 8
    HW, n, R = H * W, B * C * H * W, 5 * B
    gen = torch.Generator().manual_seed(steps)
    sch = _sched("epsilon", steps)
    table = k.lms_table(sch.lms_rows(), dev)
    lat = (torch.randn(B, C, H, W, generator=gen) * sch.init_noise_sigma).to(dev)
    sample, hist = lat.reshape(-1).clone(), torch.zeros(4, n, device=dev)
    ws, ws_e = (torch.zeros(k.calg_workspace_elems(B, C, HW), device=dev, dtype=torch.float64) for _ in range(2))
    scalars, sc_e = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    state = torch.zeros(2, device=dev, dtype=torch.int32)
    t_out = torch.zeros(R, device=dev, dtype=torch.float32)
    x_next = torch.full((R * HW, cp), 3.0, device=dev, dtype=dtype)
    for i in range(steps):
        pred = calg_test._pred(gen, B * HW, ld, dtype).to(dev)
        out = torch.empty(R, C, H, W, device=dev)
        k.nhwc_to_nchw(pred, out, R, C, HW, ld)
        noise = torch.empty(B, C, H, W, device=dev)
        k.calg_dots(out, 1, B, 1, C * HW, ws_e)
        k.calg_guidance(out, noise, G, ws_e, sc_e)
        lat, x_ref = _tail(sch, i, lat, noise, R, dtype, cp)
        k.calg_dots(pred, ld, B, C, HW, ws)
        k.calg_lms_step(pred, ld, G, ws, scalars, sample, hist, table, steps, state, t_out, x_next, cp, B, C, HW)
        _check_state(sch, i, steps, R, sample, lat, x_next, x_ref, hist, state, t_out, f"calg step {i}")
        assert torch.equal(scalars, sc_e) and scalars[0].item() > 0, i


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Bn,dim", [(3, 6), (5, 320)])
def test_timestep_embed_f32(dev, dt, Bn, dim):
    from pdm import _pdmk as k
    import test_kernels_gpu as kt
    dtype = kt.DT[dt]
    freqs = torch.exp(-math.log(10000.0) * torch.arange(dim // 2, dtype=torch.float32) / (dim // 2)).to(dev)
    # integral values: the bits of the int64 entry
    ti = torch.tensor([999, 0, 500, 1, 37][:Bn], device=dev, dtype=torch.int64)
    a, b = (torch.zeros(Bn, dim, device=dev, dtype=dtype) for _ in range(2))
    k.timestep_embed(ti, freqs, a, Bn, dim)
    k.timestep_embed(ti.to(torch.float32), freqs, b, Bn, dim)
    assert torch.equal(a, b) and a.abs().max().item() > 0.5
    # fractional values (K-LMS, 100 steps) against the torch formula
    sch = _sched("epsilon", 100)
    tf = sch.timesteps[[1, 2, 50, 98, 37][:Bn]].to(dev)
    assert tf.dtype == torch.float32 and (tf != tf.round()).all()
    k.timestep_embed(tf, freqs, b, Bn, dim)
    arg = tf[:, None] * freqs[None]
    want = torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1)
    kt.close(b, want, 1e-4 if dt == "f32" else kt.TOL[dt], f"timestep_embed_f32 {dt}")
    assert not torch.equal(b, a)
    with pytest.raises(k.PdmkError):
        k.timestep_embed(tf.double(), freqs, b, Bn, dim)


@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_eager_step_accuracy_against_restatement(dev, prediction_type):
    """The project's fp32 eager step against the restatement of diffusers' scheduler run in fp64, over 10 steps from seeded
    predictions; the yardstick is the same restatement run in fp32 (diffusers' own arithmetic), and the bound 4 x its max abs
    error: the project's chain (fused derivative coefficients, axpby forms) is ordered differently but is no longer.
    Measured on an MI355X (max abs error over all steps, fp32 restatement / project): epsilon 1.158e-05 / 1.285e-05,
    v_prediction 2.051e-06 / 2.400e-06 (profiles/lms_parity.txt)."""
    steps = 10
    _, lat, preds, want = LF.seeded_run(prediction_type, torch.float64, steps)
    _, lat32, _, ref32 = LF.seeded_run(prediction_type, torch.float32, steps)
    assert torch.equal(lat, lat32)
    err_ref = max((a.double() - b).abs().max().item() for a, b in zip(ref32, want))
    sch = _sched(prediction_type, steps)
    x, err = lat.to(dev), 0.0
    for i in range(steps):
        x = sch.step(preds[i].to(dev), sch.timesteps[i].item(), x, return_dict=False)[0]
        err = max(err, (x.cpu().double() - want[i]).abs().max().item())
    line = f"lms parity {prediction_type}: fp32 restatement max abs err {err_ref:.3e}, project fp32 eager step {err:.3e}"
    print(line)
    assert err_ref > 0 and err <= 4 * err_ref, line


def _tiny_pipe(dev, dtype):
    from pdm.pipelines.pruning_pipelines import LMSDiscreteScheduler
    import test_plms_step_gpu as plms_test
    pipe = plms_test._tiny_pipe(dev, dtype)
    pipe.scheduler = LMSDiscreteScheduler(prediction_type="v_prediction")
    return pipe


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("guidance", [7.5, 1.0])
def test_captured_lms_loop_equals_eager_tiny(dev, dtype, Bn, guidance):
    pipe = _tiny_pipe(dev, dtype)
    gen = torch.Generator().manual_seed(Bn)
    ctx = pipe.unet.cfg.cross_attention_dim
    before = pipe.captures
    for batch in range(2):                            # the second call replays the first one's capture
        pe, ne = torch.randn(Bn, 13, ctx, generator=gen), torch.randn(Bn, 13, ctx, generator=gen)
        lat = torch.randn(Bn, 4, 16, 16, generator=gen)
        kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=5, guidance_scale=guidance,
                  output_type="latent")
        e = pipe(graph=False, **kw).images
        c = pipe(**kw).images
        assert torch.equal(e, c) and torch.isfinite(c).all(), batch
        assert pipe.captures == before + 1, "one capture per shape, reused by the second call"
    # the initial noise was scaled: the latents differ from what the same call leaves under sigma 1
    assert pipe.scheduler.init_noise_sigma == float(pipe.scheduler.sigmas[0]) > 14


def test_generate_images_script_with_lms(dev, tmp_path):
    import importlib.util
    import test_fid_images_gpu as fid_test
    spec = importlib.util.spec_from_file_location("generate_images_lms_gpu", os.path.join(
        ROOT, "unlearn-ft_amd", "scripts", "baselines", "unified_concept_editing", "generate_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path, ck2, snap = fid_test._setup(tmp_path, bs=2)
    prompts = os.path.join(str(tmp_path), "prompts.csv")
    with open(prompts, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["case_number", "prompt", "evaluation_seed"])
        for c, t in {0: "a red thing", 1: "the blue one"}.items():
            w.writerow([c, t, 1000 + c])

    def run(name, extra):
        save = os.path.join(str(tmp_path), name)
        written = mod.main(["--model_name", "original", "--prompts_path", prompts, "--save_path", save, "--num_samples", "2",
                            "--ddim_steps", "3", "--image_size", "64", "--base_config_path", path, "--model_id", snap,
                            "--ckpt_path", ck2, "--tiny"] + extra)
        folder = os.path.join(save, "original")
        names = [f"{c}_{n}.png" for c in (0, 1) for n in range(2)]
        assert sorted(os.listdir(folder)) == names and written == [os.path.join(folder, n) for n in names]
        return [open(os.path.join(folder, n), "rb").read() for n in names]

    lms = run("lms", ["--scheduler", "lms"])
    default = run("default", [])
    pndm = run("pndm", ["--scheduler", "pndm"])
    assert default == pndm, "without the flag: the PNDM sampler, bit for bit"
    assert all(a != b for a, b in zip(lms, pndm)), "the flag selects another sampler"
    from PIL import Image
    import io
    for png in lms:
        with Image.open(io.BytesIO(png)) as im:
            assert im.format == "PNG" and im.mode == "RGB" and im.size == (64, 64) and np.asarray(im).std() > 0
