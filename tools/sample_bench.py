#!/usr/bin/env python3
"""Time the image-logging / FID sampler on one MI355X: B prompts, PNDM (or --scheduler lms: K-LMS),
CFG 7.5, 512 x 512, bf16, pruned student (MAC budget 0.55) + VAE decode.  Reports s / batch, images/s and the U-Net forward
rate.  --graph: the denoising loop as replays of the captured step (pdmk_plms_step / pdmk_lms_step), else the eager loop.
--neuron_masks (with --scheduler ddim or pndm): ConceptPrune's neuron removal - per-timestep masks from seeded
random norms at --skill_ratio, the time of building them, and the same loop plain and with neuron_masks=, alternating in one
process, latents out (no VAE decode in the timed window)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unlearn-ft_amd"))
from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget, plan_macs  # noqa: E402
from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned  # noqa: E402
from pdm.models.vae.autoencoder_kl import AutoencoderKL  # noqa: E402
from pdm.models.clip.text_encoder import CLIPTextModel  # noqa: E402
from pdm.pipelines.pruning_pipelines import DDIMScheduler, LMSDiscreteScheduler, StableDiffusionPruningPipeline  # noqa: E402


def neuron_masks_legs(pipe, unet, a, ids, empty, ratio):
    """Mask building, then --reps rounds of (plain, masked) sampling with one seed, each leg timed to a device synchronise."""
    from pdm.utils import concept_prune as CP
    dev = unet.device
    layers = CP.ffn_layers(unet)
    g = torch.Generator(device=dev).manual_seed(1)
    base = [torch.rand(a.steps, F, device=dev, generator=g) + 0.1 for _k, _o, F, _fp in layers]
    target = [nb * torch.exp(0.5 * torch.randn(nb.shape, device=dev, generator=g)) for nb in base]
    CP.TimestepMasks.from_norms(unet, base, target, a.skill_ratio)                  # first launches load the code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    masks = CP.TimestepMasks.from_norms(unet, base, target, a.skill_ratio)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    weights = sum(o * f for _k, o, f, _fp in layers)
    dens = [sum(v) / len(v) for v in masks.density().values()]
    print(f"neuron masks: {len(layers)} ff.net.2 layers, {weights / 1e6:.1f} M weights, T = {a.steps}, skill_ratio {a.skill_ratio}: built in "
          f"{t_build * 1e3:.1f} ms ({len(layers)} pdmk_wanda_select launches, buffers included); bits {masks.bits.numel() * 4 / 1e6:.1f} MB, "
          f"pristine copy {masks._src.numel() * masks._src.element_size() / 1e6:.1f} MB; mean density {sum(dens) / len(dens):.4f}")

    def leg(m):
        gen = torch.Generator(device=dev).manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat = pipe(prompt_ids=ids, negative_prompt_ids=empty, num_inference_steps=a.steps, generator=gen, output_type="latent",
                   graph=a.graph, neuron_masks=m).images
        torch.cuda.synchronize()
        return time.perf_counter() - t0, lat
    for m in (None, masks):                                                          # warm-up: GEMM plans and both captures
        leg(m)
    times = {"plain": [], "masked": []}
    for r in range(a.reps):
        for name in (("plain", "masked") if r % 2 == 0 else ("masked", "plain")):
            el, lat = leg(masks if name == "masked" else None)
            times[name].append(el)
    calls = a.steps + (1 if a.scheduler == "pndm" else 0)
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    for n in ("plain", "masked"):
        print(f"sampler {'captured' if a.graph else 'eager'} B={a.batch} {a.steps} {a.scheduler.upper()} steps ({calls} U-Net calls on 2B), CFG 7.5, "
              f"512x512, bf16, budget {ratio:.3f}, latents out, {n}: median of {a.reps} {med[n] * 1e3:.1f} ms = {med[n] / calls * 1e3:.3f} ms per call "
              f"(runs: {' '.join(f'{t * 1e3:.1f}' for t in times[n])})")
    print(f"neuron_masks cost: {(med['masked'] - med['plain']) / calls * 1e6:+.1f} us per U-Net call = "
          f"{(med['masked'] / med['plain'] - 1) * 100:+.2f} % of the loop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--budget", type=float, default=0.55)
    ap.add_argument("--graph", action="store_true", help="captured denoising loop (the capture happens in the warm-up)")
    ap.add_argument("--reps", type=int, default=1, help="timed batches (the mean is reported)")
    ap.add_argument("--scheduler", choices=["pndm", "lms", "ddim"], default="pndm", help="lms: K-LMS (pdmk_lms_step when --graph)")
    ap.add_argument("--neuron_masks", action="store_true", help="plain against neuron_masks= (ddim / pndm), alternating")
    ap.add_argument("--skill_ratio", type=float, default=0.01)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = UNetConfig.sd21()
    av, ratio, _ = arch_vector_for_budget(cfg, a.budget, hw=64)
    unet = UNet2DConditionModelPruned(cfg, av, dev, torch.bfloat16, train=False, seed=0)
    vae = AutoencoderKL(None, dev, torch.bfloat16, seed=0)
    txt = CLIPTextModel(None, dev, torch.bfloat16, seed=0)
    sched = {"lms": LMSDiscreteScheduler, "ddim": DDIMScheduler}.get(a.scheduler)
    pipe = StableDiffusionPruningPipeline(vae, txt, unet, sched() if sched else None)
    ids = torch.randint(0, 49408, (a.batch, 77), device=dev)
    empty = torch.zeros(a.batch, 77, dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    if a.neuron_masks:
        return neuron_masks_legs(pipe, unet, a, ids, empty, ratio)
    pipe(prompt_ids=ids, negative_prompt_ids=empty, num_inference_steps=a.steps if a.graph else 2, generator=gen,
         graph=a.graph)                                                       # warm-up: GEMM plans (and the capture)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        img = pipe(prompt_ids=ids, negative_prompt_ids=empty, num_inference_steps=a.steps, generator=gen, output_type="pt",
                   graph=a.graph).images
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / a.reps
    macs = plan_macs(cfg, unet.blocks, 64, 77)[0]
    calls = a.steps + 1 if a.scheduler == "pndm" else a.steps
    print(f"sampler {'captured' if a.graph else 'eager'} B={a.batch} {a.steps} {a.scheduler.upper()} steps ({calls} U-Net calls on 2B), CFG 7.5, 512x512, bf16, budget {ratio:.3f}: "
          f"{el:.2f} s/batch = {a.batch / el:.2f} img/s; U-Net {2 * macs * 2 * a.batch * calls / el / 1e12:.0f} TFLOP/s incl. "
          f"text encode + VAE decode; image range [{img.min().item():.2f}, {img.max().item():.2f}]")


if __name__ == "__main__":
    main()
