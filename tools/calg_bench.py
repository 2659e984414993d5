#!/usr/bin/env python3
"""What concept algebra costs in the sampler, on one MI355X (modelled on tools/sld_bench.py).

Part 1, the step alone: B = 10, 4 x 64 x 64 latents, bf16 predictions, 50 PNDM steps (51 launches per schedule).  The same random
latents and prediction rows go through
    plain    pdmk_plms_step on 2B rows (the parent's launch)
    calg     pdmk_calg_dots + pdmk_calg_plms_step on 5B rows
timed with device events around one whole schedule, --rounds alternating rounds after a warm-up; microseconds per launch pair.

Part 2, a sampling run: random weights of SD-2.1 shapes, dense and at MAC budget 0.55, bf16, B = 1, 50 PNDM steps at 512 x 512
(64 x 64 latents, 77 x 1024 text states), latents out - the denoising loop alone.  Per topology, after a warm-up of every form,
--rounds alternating rounds of
    plain     two-branch guidance, captured (2B U-Net batch + pdmk_plms_step)
    calg      concept algebra, captured (5B U-Net batch + pdmk_calg_dots + pdmk_calg_plms_step)
    calg-eag  concept algebra, eager loop (5B U-Net call + pdmk_calg_dots + pdmk_calg_guidance + PNDMScheduler.step)
each timed by a host clock around one whole call that ends in a device synchronise.  Lines go to stdout and, with --out, to that
file (profiles/calg_bench.txt).  Nothing is asserted; captured and eager outputs are compared bit for bit and reported."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unlearn-ft_amd"))
import torch
from pdm import _pdmk as k
from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget, padc
from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
from pdm.pipelines.pruning_pipelines import PNDMScheduler, StableDiffusionPruningPipeline

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


# ---- part 1: the step launches alone
B, C, H, W, G = 10, 4, 64, 64, 7.5
HW, n, cp = H * W, B * C * H * W, padc(C)
gen = torch.Generator().manual_seed(0)
sch = PNDMScheduler(prediction_type="v_prediction")
sch.set_timesteps(args.steps)
rows = sch.plms_rows()
N = len(rows)
table = k.plms_table(rows, dev)
lat = torch.randn(n, generator=gen).to(dev)
pred = (torch.randn(5 * B * HW, cp, generator=gen) * 2).to(torch.bfloat16).to(dev)
sample, cur, ets = lat.clone(), torch.zeros(n, device=dev), torch.zeros(4, n, device=dev)
state = torch.zeros(2, device=dev, dtype=torch.int32)
t_out = torch.zeros(5 * B, device=dev, dtype=torch.int64)
x_next = torch.zeros(5 * B * HW, cp, device=dev, dtype=torch.bfloat16)
ws = torch.zeros(k.calg_workspace_elems(B, C, HW), device=dev, dtype=torch.float64)
scalars = torch.zeros(2, device=dev)


def schedule(form):
    sample.copy_(lat)
    state.zero_()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(N):
        if form == "plain":
            k.plms_step(pred, cp, 1.0 - G, G, True, sample, cur, ets, table, N, state, t_out, x_next, cp, B, C, HW)
        else:
            k.calg_dots(pred, cp, B, C, HW, ws)
            k.calg_plms_step(pred, cp, G, ws, scalars, sample, cur, ets, table, N, state, t_out, x_next, cp, B, C, HW)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / N


say(f"# calg_bench: {torch.cuda.get_device_name(0)}")
say(f"# part 1: the step alone, B = {B}, {C} x {H} x {W} latents ({n} elements), bf16 rows, {args.steps} PNDM steps = {N} launches per "
    f"schedule, device events around a schedule; us per U-Net call's step work, {args.rounds} alternating rounds after one warm-up each")
for form in ("plain", "calg"):
    schedule(form)
best = {"plain": [], "calg": []}
for rnd in range(args.rounds):
    for form in best:
        best[form].append(schedule(form))
    say(f"   round {rnd}: plain (pdmk_plms_step, 2B rows) {best['plain'][-1]:7.2f} us   calg (pdmk_calg_dots + pdmk_calg_plms_step, "
        f"5B rows) {best['calg'][-1]:7.2f} us")
say(f"   best of {args.rounds}: plain {min(best['plain']):.2f} us  calg {min(best['calg']):.2f} us  calg / plain "
    f"{min(best['calg']) / min(best['plain']):.2f}; finite: {bool(torch.isfinite(sample).all())}; nrm, dot = {scalars.tolist()}")

# ---- part 2: a sampling run
g = torch.Generator().manual_seed(0)
pe, ne = (torch.randn(1, 77, 1024, generator=g).to(dev) for _ in range(2))
concepts = torch.randn(3, 77, 1024, generator=g).to(dev)
lat = torch.randn(1, 4, 64, 64, generator=g).to(dev)
say(f"# part 2: bf16, B = 1, {args.steps} PNDM steps, 64x64 latents, guidance 7.5; ms per whole denoising loop (host clock, "
    f"synchronised), {args.rounds} alternating rounds after one warm-up each")
for topo in args.topologies.split(","):
    av = None if topo == "dense" else arch_vector_for_budget(cfg, float(topo), hw=64)[0]
    unet = UNet2DConditionModelPruned(cfg, av, dev, torch.bfloat16, train=False, seed=0)
    vae = AutoencoderKL(VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1), dev, torch.bfloat16, seed=7)   # unused: latents out
    pipe = StableDiffusionPruningPipeline(vae, None, unet, PNDMScheduler(prediction_type="v_prediction"))
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.steps, guidance_scale=7.5,
              output_type="latent")
    forms = {"plain": lambda: pipe(graph=True, **kw).images,
             "calg": lambda: pipe(graph=True, algebra_embeds=concepts, **kw).images,
             "calg-eag": lambda: pipe(graph=False, algebra_embeds=concepts, **kw).images}
    warm = {name: timed(fn) for name, fn in forms.items()}
    say(f"== {topo}: {unet.num_parameters() / 1e6:.1f} M parameters; warm-up (plans, captures) " +
        "  ".join(f"{n_} {t:9.1f} ms" for n_, (t, _) in warm.items()))
    say(f"   captured == eager bit for bit: {torch.equal(warm['calg'][1], warm['calg-eag'][1])}; "
        f"finite: {bool(torch.isfinite(warm['calg'][1]).all())}; differs from plain: {not torch.equal(warm['calg'][1], warm['plain'][1])}")
    times = {n_: [] for n_ in forms}
    for rnd in range(args.rounds):
        for name, fn in forms.items():
            times[name].append(timed(fn)[0])
        say(f"   round {rnd}: " + "  ".join(f"{n_} {times[n_][-1]:9.1f} ms" for n_ in forms))
    best = {n_: min(v) for n_, v in times.items()}
    calls = args.steps + 1
    say(f"   best of {args.rounds}: plain {best['plain']:.1f} ms ({best['plain'] / calls:.2f} per U-Net call on 2 rows)  calg "
        f"{best['calg']:.1f} ms ({best['calg'] / calls:.2f} per call on 5 rows)  calg / plain {best['calg'] / best['plain']:.3f} "
        f"(rows 5 / 2 = 2.5)  calg eager / calg captured {best['calg-eag'] / best['calg']:.3f}")
    del pipe, unet, vae, forms, warm
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
