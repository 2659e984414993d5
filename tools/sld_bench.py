#!/usr/bin/env python3
"""What Safe Latent Diffusion costs in the sampler, on one MI355X: random weights of SD-2.1 shapes, dense and at MAC budget 0.55,
bf16, B = 1, 50 PNDM steps (51 U-Net calls) at 512 x 512 (64 x 64 latents, 77 x 1024 text states), latents out - the denoising
loop alone, no text encoder and no VAE.  Per topology, after a warm-up of every form (GEMM plans, the two captures), --rounds
alternating rounds of
    plain    two-branch guidance, captured (2B U-Net batch + pdmk_plms_step)
    sld      SLD Medium, captured (3B U-Net batch + pdmk_sld_plms_step)
    sld-eag  SLD Medium, eager loop (3B U-Net call + pdmk_sld_guidance + PNDMScheduler.step)
each timed by a host clock around one whole call that ends in a device synchronise.  Lines go to stdout and, with --out, to that
file (profiles/sld_bench.txt).  Nothing is asserted; the outputs of captured and eager SLD are compared bit for bit and reported."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unlearn-ft_amd"))
import torch
from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget
from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
from pdm.pipelines.pruning_pipelines import PNDMScheduler, StableDiffusionPruningPipeline
from pdm.utils import sld

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--topologies", default="dense,0.55")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = UNetConfig.sd21()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


g = torch.Generator().manual_seed(0)
pe, ne, se = (torch.randn(1, 77, 1024, generator=g).to(dev) for _ in range(3))
lat = torch.randn(1, 4, 64, 64, generator=g).to(dev)
medium = sld.preset("Medium")
say(f"# sld_bench: {torch.cuda.get_device_name(0)}, bf16, B = 1, {args.steps} PNDM steps, 64x64 latents, guidance 7.5, SLD Medium "
    f"{medium}; ms per whole denoising loop (host clock, synchronised), {args.rounds} alternating rounds after one warm-up each")
for topo in args.topologies.split(","):
    av = None if topo == "dense" else arch_vector_for_budget(cfg, float(topo), hw=64)[0]
    unet = UNet2DConditionModelPruned(cfg, av, dev, torch.bfloat16, train=False, seed=0)
    vae = AutoencoderKL(VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1), dev, torch.bfloat16, seed=7)   # unused: latents out
    pipe = StableDiffusionPruningPipeline(vae, None, unet, PNDMScheduler(prediction_type="v_prediction"))
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.steps, guidance_scale=7.5,
              output_type="latent")
    forms = {"plain": lambda: pipe(graph=True, **kw).images,
             "sld": lambda: pipe(graph=True, safety_concept_embeds=se, **medium, **kw).images,
             "sld-eag": lambda: pipe(graph=False, safety_concept_embeds=se, **medium, **kw).images}
    warm = {name: timed(fn) for name, fn in forms.items()}
    say(f"== {topo}: {unet.num_parameters() / 1e6:.1f} M parameters; warm-up (plans, captures) " +
        "  ".join(f"{n} {t:9.1f} ms" for n, (t, _) in warm.items()))
    say(f"   captured SLD == eager SLD bit for bit: {torch.equal(warm['sld'][1], warm['sld-eag'][1])}; "
        f"finite: {bool(torch.isfinite(warm['sld'][1]).all())}; differs from plain: {not torch.equal(warm['sld'][1], warm['plain'][1])}")
    times = {n: [] for n in forms}
    for rnd in range(args.rounds):
        for name, fn in forms.items():
            times[name].append(timed(fn)[0])
        say(f"   round {rnd}: " + "  ".join(f"{n} {times[n][-1]:9.1f} ms" for n in forms))
    best = {n: min(v) for n, v in times.items()}
    calls = args.steps + 1
    say(f"   best of {args.rounds}: plain {best['plain']:.1f} ms ({best['plain'] / calls:.2f} per U-Net call on 2 rows)  sld "
        f"{best['sld']:.1f} ms ({best['sld'] / calls:.2f} per call on 3 rows)  sld / plain {best['sld'] / best['plain']:.3f} "
        f"(rows 3 / 2 = 1.5)  sld eager / sld captured {best['sld-eag'] / best['sld']:.3f}")
    del pipe, unet, vae, forms, warm
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
