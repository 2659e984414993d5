"""pdmk_plms_step and pdmk_image_to_u8 (csrc/sampler.hip, -m gpu): bit-identical to the eager chain they replace, and the
captured denoising loop of StableDiffusionPruningPipeline bit-identical to the eager loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _eager_chain(sch, pred, ld, B, C, H, W, cfg, g, lat, dtype, cp):
    """What generate_samples' eager loop does between two U-Net calls: NHWC -> NCHW, guidance axpby, PNDMScheduler.step,
    the doubled latent copy and nchw_to_nhwc.  Returns (new latents, next U-Net input)."""
    from pdm import _pdmk as k
    R = 2 * B if cfg else B
    out = torch.empty(R, C, H, W, device=lat.device)
    k.nhwc_to_nchw(pred, out, R, C, H * W, ld)
    if cfg:
        noise = out[B:]
        k.axpby(out[:B], noise, 1.0 - g, g)
    else:
        noise = out
    lat = sch.step(noise.contiguous(), int(sch.timesteps[sch.counter]), lat, return_dict=False)[0]
    x2 = torch.cat([lat, lat]) if cfg else lat
    x = torch.empty(R * H * W, cp, device=lat.device, dtype=dtype)
    k.nchw_to_nhwc(x2.contiguous(), x, R, C, H * W, cp)
    return lat, x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_plms_step_equals_eager_chain(dev, dtype, cfg, prediction_type):
    from pdm import _pdmk as k
    from pdm.pipelines.pruning_pipelines import PNDMScheduler
    from pdm.models.unet.spec import padc
    B, C, H, W, g = 2, 4, 8, 12, 7.5
    cp, ld = padc(C), padc(C) + 8                     # the prediction's row stride differs from the input's
    R = 2 * B if cfg else B
    n = B * C * H * W
    for steps in (1, 2, 3, 10, 50):
        gen = torch.Generator(device=dev).manual_seed(steps)
        sch = PNDMScheduler(prediction_type=prediction_type)
        sch.set_timesteps(steps)
        rows = sch.plms_rows()
        N = len(rows)
        table = k.plms_table(rows, dev)
        lat0 = torch.randn(B, C, H, W, device=dev, generator=gen)
        sample, cur, ets = lat0.reshape(-1).clone(), torch.zeros(n, device=dev), torch.zeros(4, n, device=dev)
        state = torch.zeros(2, device=dev, dtype=torch.int32)
        t_out = torch.zeros(R, device=dev, dtype=torch.int64)
        x_next = torch.full((R * H * W, cp), 3.0, device=dev, dtype=dtype)      # padding must come back as zeros
        lat = lat0.clone()
        appended = 0
        for i in range(N):
            pred = (torch.randn(R * H * W, ld, device=dev, generator=gen) * 2).to(dtype)
            lat, x_ref = _eager_chain(sch, pred, ld, B, C, H, W, cfg, g, lat, dtype, cp)
            k.plms_step(pred, ld, 1.0 - g, g, cfg, sample, cur, ets, table, N, state, t_out, x_next, cp, B, C, H * W)
            what = f"steps {steps}, step {i}"
            assert torch.equal(sample.view(B, C, H, W), lat), what
            assert torch.equal(x_next, x_ref), what
            assert state.tolist() == [i + 1, 0], what
            if i + 1 < N:
                assert t_out.tolist() == [int(sch.timesteps[i + 1])] * R, what
            if i != 1:
                appended += 1
            for j, e in enumerate(reversed(sch.ets)):           # history: ets[-1 - j] lives in ring slot (appended - 1 - j) % 4
                assert torch.equal(ets[(appended - 1 - j) % 4].view(B, C, H, W), e), (what, j)
            if sch.cur_sample is not None:
                assert torch.equal(cur.view(B, C, H, W), sch.cur_sample), what
        # a launch past the end of the table changes nothing
        before = [t.clone() for t in (sample, ets, x_next, state)]
        k.plms_step(pred, ld, 1.0 - g, g, cfg, sample, cur, ets, table, N, state, t_out, x_next, cp, B, C, H * W)
        assert all(torch.equal(a, b) for a, b in zip(before, (sample, ets, x_next, state)))


def test_image_to_u8_equals_numpy_truncation(dev):
    from pdm import _pdmk as k
    gen = torch.Generator().manual_seed(0)
    B, C, H, W = 3, 3, 17, 23
    x = torch.randn(B, C, H, W, generator=gen) * 1.2
    flat = x.view(-1)
    m = torch.arange(256, dtype=torch.float32)
    special = torch.cat([torch.tensor([1.0, -1.0, 1.0000001, -1.0000001, 1.5, -1.5, 0.0, -0.0]),
                         (m / 255) * 2 - 1,                                  # x / 2 + 0.5 = m / 255 (to fp32 rounding)
                         m / 255, -(m / 255)])
    flat[:special.numel()] = special
    want = ((x.to(dev) / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).cpu().numpy() * 255).astype(np.uint8)
    got = torch.empty(B, H, W, C, device=dev, dtype=torch.uint8)
    k.image_to_u8(x.to(dev).contiguous(), got)
    assert np.array_equal(got.cpu().numpy(), want)


def _tiny_pipe(dev, dtype, tokenizer=None):
    from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
    from pdm.pipelines.pruning_pipelines import StableDiffusionPruningPipeline, PNDMScheduler
    cfg = UNetConfig.tiny()
    av = arch_vector_for_budget(cfg, 0.6, hw=16)[0]
    unet = UNet2DConditionModelPruned(cfg, av, dev, dtype, train=False, seed=0)
    vae = AutoencoderKL(VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1), dev, dtype, seed=7)
    return StableDiffusionPruningPipeline(vae, None, unet, PNDMScheduler(prediction_type="v_prediction"), tokenizer)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("guidance", [7.5, 1.0])
def test_captured_loop_equals_eager_tiny(dev, dtype, B, guidance):
    pipe = _tiny_pipe(dev, dtype)
    gen = torch.Generator().manual_seed(B)
    ctx = pipe.unet.cfg.cross_attention_dim
    for steps in (3, 10):
        before = pipe.captures
        for batch in range(2):                        # the second batch replays the first one's capture
            pe, ne = torch.randn(B, 13, ctx, generator=gen), torch.randn(B, 13, ctx, generator=gen)
            lat = torch.randn(B, 4, 16, 16, generator=gen)
            kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=steps,
                      guidance_scale=guidance)
            for out in ("latent", "pt"):
                e = pipe(graph=False, output_type=out, **kw).images
                c = pipe(output_type=out, **kw).images
                assert torch.equal(e, c), (steps, batch, out)
        assert pipe.captures == before + 1, "one capture per shape, reused by the next batch"


def test_captured_loop_equals_eager_fullsize(dev):
    """SD-2.1 student at MAC budget 0.55, 64 x 64 latents, bf16, B = 1, 4 PNDM steps with guidance."""
    from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
    from pdm.pipelines.pruning_pipelines import StableDiffusionPruningPipeline, PNDMScheduler
    cfg = UNetConfig.sd21()
    av = arch_vector_for_budget(cfg, 0.55, hw=64)[0]
    unet = UNet2DConditionModelPruned(cfg, av, dev, torch.bfloat16, train=False, seed=0)
    vae = AutoencoderKL(VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1), dev, torch.bfloat16, seed=7)
    pipe = StableDiffusionPruningPipeline(vae, None, unet, PNDMScheduler(prediction_type="v_prediction"))
    gen = torch.Generator().manual_seed(5)
    pe, ne = torch.randn(1, 77, 1024, generator=gen), torch.randn(1, 77, 1024, generator=gen)
    lat = torch.randn(1, 4, 64, 64, generator=gen)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=4, output_type="latent")
    e = pipe(graph=False, **kw).images
    c = pipe(**kw).images
    assert pipe.captures == 1 and torch.equal(e, c)


def test_string_prompts_equal_token_ids(dev, tmp_path):
    import data_fixtures as F
    from pdm.models.clip.text_encoder import CLIPTextModel, CLIPTextConfig
    from pdm.utils.data import load_tokenizer, tokenize
    tok = load_tokenizer(F.write_tokenizer(str(tmp_path)))
    pipe = _tiny_pipe(dev, torch.bfloat16, tokenizer=tok)
    ctx = pipe.unet.cfg.cross_attention_dim
    pipe.text_encoder = CLIPTextModel(CLIPTextConfig(vocab_size=1000, hidden_size=ctx, intermediate_size=256,
                                                     num_hidden_layers=2, num_attention_heads=ctx // 64),
                                      dev, torch.bfloat16, seed=3)
    prompts = ["a photo of the thing", "and the other one"]
    lat = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(9))
    a = pipe(prompt=prompts, latents=lat, num_inference_steps=3, output_type="latent").images
    b = pipe(prompt_ids=tokenize(tok, prompts).to(dev), negative_prompt_ids=tokenize(tok, ["", ""]).to(dev), latents=lat,
             num_inference_steps=3, output_type="latent").images
    assert torch.equal(a, b)
    u8 = pipe(prompt=prompts, latents=lat, num_inference_steps=3, output_type="u8").images
    f = pipe(prompt=prompts, latents=lat, num_inference_steps=3, output_type="np").images
    assert u8.dtype == np.uint8 and np.array_equal(u8, (f * 255).astype(np.uint8))
