"""Safe Latent Diffusion in StableDiffusionPruningPipeline.generate_samples (-m gpu), on the tiny pipeline of
tests/test_plms_step_gpu.py: the captured 3B loop bit-identical to the eager one, SLD off bit-identical to a plain call, the
degenerate concept against a host loop, and a live safety branch."""
import pytest
import torch

import test_plms_step_gpu as plms_test            # its tiny pipeline

pytestmark = pytest.mark.gpu
MEDIUM = dict(sld_guidance_scale=1000, sld_warmup_steps=10, sld_threshold=0.01, sld_momentum_scale=0.3, sld_mom_beta=0.4)
MAX = dict(sld_guidance_scale=5000, sld_warmup_steps=0, sld_threshold=1.0, sld_momentum_scale=0.5, sld_mom_beta=0.7)
T = 13


def _pipe(dev, dtype, kind):
    from pdm.pipelines.pruning_pipelines import DDIMScheduler
    pipe = plms_test._tiny_pipe(dev, dtype)
    if kind == "ddim":
        pipe.scheduler = DDIMScheduler(prediction_type="v_prediction")
    return pipe


def _batch(pipe, B, gen, steps):
    ctx = pipe.unet.cfg.cross_attention_dim
    return dict(prompt_embeds=torch.randn(B, T, ctx, generator=gen), negative_prompt_embeds=torch.randn(B, T, ctx, generator=gen),
                latents=torch.randn(B, 4, 16, 16, generator=gen), num_inference_steps=steps)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_captured_sld_loop_equals_eager(dev, kind, B, dtype):
    pipe = _pipe(dev, dtype, kind)
    gen = torch.Generator().manual_seed(B)
    ctx = pipe.unet.cfg.cross_attention_dim
    for steps in (3, 12):                                 # 12: both sides of Medium's warm-up
        before = pipe.captures
        for batch in range(2):                            # the second batch replays the first one's capture
            kw = dict(_batch(pipe, B, gen, steps), safety_concept_embeds=torch.randn(1, T, ctx, generator=gen), **MEDIUM)
            for out in ("latent", "pt"):
                e = pipe(graph=False, output_type=out, **kw).images
                c = pipe(graph=True, output_type=out, **kw).images
                assert torch.equal(e, c), (steps, batch, out)
        assert pipe.captures == before + 1, "one capture per shape, reused by the next batch"


@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_sld_off_changes_nothing(dev, kind):
    pipe = _pipe(dev, torch.bfloat16, kind)
    gen = torch.Generator().manual_seed(7)
    ctx = pipe.unet.cfg.cross_attention_dim
    kw = dict(_batch(pipe, 2, gen, 3), output_type="latent")
    concept = torch.randn(1, T, ctx, generator=gen)
    for graph in (True, False):
        plain = pipe(graph=graph, **kw).images
        captures, keys = pipe.captures, list(pipe._loops)
        if graph:
            assert captures == 1
        off = [pipe(graph=graph, safety_concept_embeds=concept, **dict(MEDIUM, sld_guidance_scale=1.0), **kw).images,
               pipe(graph=graph, **MEDIUM, **kw).images]                                         # no safety concept
        assert torch.equal(off[0], plain) and torch.equal(off[1], plain)
        assert pipe.captures == captures and list(pipe._loops) == keys, "SLD off: the plain call's loop, no new capture"
        on = pipe(graph=graph, safety_concept_embeds=concept, **MAX, **kw).images      # no warm-up: the branch acts
        assert not torch.equal(on, plain)
        assert pipe.captures == captures + int(graph) and (not graph or "sld" in list(pipe._loops)[-1])
    # without classifier-free guidance SLD is off too
    a = pipe(graph=False, **dict(kw, guidance_scale=1.0)).images
    b = pipe(graph=False, safety_concept_embeds=concept, **MEDIUM, **dict(kw, guidance_scale=1.0)).images
    assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_concept_equal_to_negative_prompt_is_plain_guidance(dev, kind):
    """s = u: d = t - u, gs = (u - u) * scale + momentum_scale * 0 = 0 whatever the scale, so pred = u + g * ((t - u) - 0).
    The host loop below is that in torch fp32 operations plus scheduler.step."""
    pipe = _pipe(dev, torch.float32, kind)
    gen = torch.Generator().manual_seed(11)
    g, steps, B = 7.5, 12, 1
    kw = _batch(pipe, B, gen, steps)
    got = pipe(graph=False, output_type="latent", guidance_scale=g, safety_concept_embeds=kw["negative_prompt_embeds"], **MAX,
               **kw).images
    sch = pipe.scheduler
    sch.set_timesteps(steps)
    lat = kw["latents"].to(dev)
    ehs = torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"], kw["negative_prompt_embeds"]]).to(dev)
    gg = torch.tensor(g, dtype=torch.float32, device=dev)
    for t in sch.timesteps.tolist():
        x = torch.cat([lat, lat, lat])
        out = pipe.unet(x, torch.full((3 * B,), t, device=dev, dtype=torch.int64), ehs, return_dict=False)[0]
        u, tx, s = out[:B], out[B:2 * B], out[2 * B:]
        assert torch.equal(u, s)                          # equal rows in, equal rows out: the U-Net does not mix the batch
        lat = sch.step((u + gg * (tx - u)).contiguous(), t, lat, return_dict=False)[0]
    assert torch.equal(got, lat)


def test_other_concept_changes_latents_and_end_iteration(dev):
    pipe = _pipe(dev, torch.bfloat16, "plms")
    gen = torch.Generator().manual_seed(13)
    ctx = pipe.unet.cfg.cross_attention_dim
    kw = dict(_batch(pipe, 2, gen, 6), output_type="latent")
    concept = torch.randn(1, T, ctx, generator=gen)
    plain = pipe(**kw).images
    safe = pipe(safety_concept_embeds=concept, **MAX, **kw).images
    assert torch.isfinite(safe).all() and not torch.equal(safe, plain)
    for end in (0, 1, 2, 5, 7):                           # U-Net calls: PNDM's repeated call is one of them
        e = pipe(graph=False, end_iteration=end, safety_concept_embeds=concept, **MAX, **kw).images
        c = pipe(graph=True, end_iteration=end, safety_concept_embeds=concept, **MAX, **kw).images
        assert torch.equal(e, c), end
    assert torch.equal(c, safe)                           # 7 calls are the whole 6-step schedule
