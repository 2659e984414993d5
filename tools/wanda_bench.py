#!/usr/bin/env python3
"""ConceptPrune kernels and the observer's cost in the sampler.
  1. pdmk_rownorm_colsq at the (M, F) of the dense SD-2.1 feed-forward blocks with guidance (M = 2 H W) at 512^2 and 768^2, bf16,
     graph-timed; bytes of x read once over time (the kernel reads x twice: the second read is the figure's other half) against
     a plain copy of the same tensor.
  2. pdmk_wanda_count at (O, F, T) of the dense blocks, fp32 weights, device events around 3 launches.
  3. the sampler at B = 1, --steps steps, guidance 7.5, DDIM eager loop on the dense topology (random weights), with and
     without a WandaObserver (--no-sampler skips it, --res the image size).
One line per measurement; nothing is asserted."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unlearn-ft_amd"))
import torch
from pdm import _pdmk as k

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--no-sampler", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
REP = 10


def gtime(fn):
    """us per call: REP calls captured in one graph, five replays between two events."""
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REP): fn()
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5): g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (5 * REP) * 1e3


print("== pdmk_rownorm_colsq, bf16 (M = 2 H W, F = 4 C)")
for res in (512, 768):
    for lvl, C in enumerate((320, 640, 1280, 1280)):
        side = res // 8 >> lvl
        M, F = 2 * side * side, 4 * C
        x = torch.randn(M, F, device=dev).to(torch.bfloat16)
        y = torch.empty_like(x)
        acc = torch.zeros(F, device=dev)
        t = gtime(lambda: k.rownorm_colsq(x, acc))
        tc = gtime(lambda: y.copy_(x))
        nb = M * F * 2
        print(f"{res}^2 M{M:6d} F{F:5d}: {t:7.1f} us  ({nb / t / 1e6:5.2f} TB/s of x once, {2 * nb / t / 1e6:5.2f} TB/s of its two reads)   "
              f"copy {tc:6.1f} us ({2 * nb / tc / 1e6:5.2f} TB/s of 1R+1W)", flush=True)

print("== pdmk_wanda_count, fp32 weights, k = int(0.01 F)")
for O, F, T in ((1280, 5120, 50), (640, 2560, 50), (320, 1280, 50)):
    g = torch.Generator(device=dev).manual_seed(0)
    w = torch.randn(O, F, device=dev, generator=g)
    nb_ = torch.rand(T, F, device=dev, generator=g) + 0.1
    nt = nb_ * torch.exp(0.5 * torch.randn(T, F, device=dev, generator=g))
    count = torch.zeros(O, F, device=dev, dtype=torch.int32)
    k.wanda_count(w, nb_, nt, int(0.01 * F), count); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3): k.wanda_count(w, nb_, nt, int(0.01 * F), count)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 3
    print(f"O{O} F{F} T{T}: {ms:8.3f} ms per launch  ({ms * 1e3 / (O * T):6.2f} us per row and timestep; density of count > 0 "
          f"{float((count > 0).float().mean()):.3f})", flush=True)

if not args.no_sampler:
    from pdm.models.unet.spec import UNetConfig
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    from pdm.models.vae.autoencoder_kl import AutoencoderKL
    from pdm.pipelines.pruning_pipelines import DDIMScheduler, StableDiffusionPruningPipeline
    from pdm.utils import concept_prune as CP
    print(f"== sampler, dense SD-2.1 topology (random weights), bf16, B = 1, {args.steps} DDIM steps, guidance 7.5, {args.res}^2, "
          f"latents out (no VAE decode)")
    cfg = UNetConfig.sd21()
    unet = UNet2DConditionModelPruned(cfg, None, dev, torch.bfloat16, train=False, seed=0)
    vae = AutoencoderKL.from_pretrained(None, subfolder="vae", random_init=True, torch_dtype=torch.bfloat16, device=dev)
    pipe = StableDiffusionPruningPipeline(vae, None, unet, DDIMScheduler(prediction_type="v_prediction"))
    g = torch.Generator().manual_seed(0)
    pe, ne = torch.randn(1, 77, cfg.cross_attention_dim, generator=g), torch.randn(1, 77, cfg.cross_attention_dim, generator=g)
    lat = torch.randn(1, 4, args.res // 8, args.res // 8, generator=g)
    obs = CP.WandaObserver(unet, args.steps)

    def run(observer):
        obs.reset_time_layer()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with CP.observing(unet, observer):
            pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.steps, guidance_scale=7.5,
                 output_type="latent")
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    run(None); run(obs)                     # warm-up of both (GEMM plans, workspaces)
    for rnd in range(3):                    # alternating
        a, b = run(None), run(obs)
        print(f"round {rnd}: no observer {a:6.3f} s ({1 / a:5.3f} images/s)   observer {b:6.3f} s ({1 / b:5.3f} images/s)   "
              f"+{(b - a) * 1e3:6.1f} ms = {(b - a) * 1e6 / (args.steps * obs.L):5.1f} us per observed layer call", flush=True)
