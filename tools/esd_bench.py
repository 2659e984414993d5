#!/usr/bin/env python3
"""ESD's iteration on one MI355X: random weights of SD-2.1 shapes at MAC budget 0.55, 64 x 64 latents, 77 x 1024 text states.
  1. per train method (xattn, noxattn) and dtype (bf16, fp32): the parts of an iteration at `iteration` = 24 - partial sampling
     (captured), frozen forward (3 rows), student forward + head + backward, optimiser + refresh - then whole iterations over
     --draws seeded draws (pdm.utils.esd.draws) and the projection to the reference's 1000 iterations.
  2. partial sampling (24 steps) captured against eager, alternated in the same run, three rounds.
  3. pdmk_adamw_segments on the xattn / noxattn table against pdmk_adamw on one contiguous range of the same element count.
One line per measurement; nothing is asserted."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unlearn-ft_amd"))
import numpy as np
import torch
from pdm import _pdmk as k
from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget
from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
from pdm.pipelines.pruning_pipelines import DDIMScheduler, StableDiffusionPruningPipeline
from pdm.training.esd import EsdTrainer
from pdm.utils import esd as E

ap = argparse.ArgumentParser()
ap.add_argument("--draws", type=int, default=50)
ap.add_argument("--dtypes", default="bf16,fp32")
ap.add_argument("--methods", default="xattn,noxattn")
ap.add_argument("--iteration", type=int, default=24)
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = UNetConfig.sd21()
av = arch_vector_for_budget(cfg, 0.55, hw=64)[0]
g = torch.Generator().manual_seed(0)
emb = {t: torch.randn(1, 77, 1024, generator=g).to(dev) for t in ("", "concept")}
lat = torch.randn(1, 4, 64, 64, generator=g)


def ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for dn in args.dtypes.split(","):
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dn]
    frozen = UNet2DConditionModelPruned(cfg, av, dev, dtype, train=False, seed=0)
    student = UNet2DConditionModelPruned(cfg, av, dev, dtype, train=True, seed=0)          # the same seed: the same weights
    vae = AutoencoderKL(VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1), dev, dtype, seed=7)
    pipe = StableDiffusionPruningPipeline(vae, None, student, DDIMScheduler(prediction_type="v_prediction"))
    print(f"== {dn}: {student.num_parameters() / 1e6:.1f} M parameters, arena {student.store.total / 1e6:.1f} M elements", flush=True)
    it = args.iteration
    for method in args.methods.split(","):
        tr = EsdTrainer(frozen, student, pipe, method, lr=1e-5)
        tr._emb.update(emb)
        n_tr = sum(n for _, n in tr.segments)
        print(f"-- {dn} {method}: {len(tr.segments)} segments, {tr.opt.table.nrows} table rows, {n_tr / 1e6:.1f} M trainable "
              f"elements", flush=True)
        x = tr.sample(emb["concept"], emb[""], lat, it)
        t = tr.t_of[it]
        t_samp = ms(lambda: tr.sample(emb["concept"], emb[""], lat, it), 2)
        t_frozen = ms(lambda: tr.frozen_predictions(x, t, emb["concept"], emb[""], emb["concept"], False))
        xin, tt, pf = tr.frozen_predictions(x, t, emb["concept"], emb[""], emb["concept"], False)
        t_student = ms(lambda: tr.student_pass(xin, tt, pf, emb["concept"], False, 4, 64, 64))
        t_opt = ms(lambda: tr.opt.step(grad_scale=1.0, zero_grad=True))
        total = t_samp + t_frozen + t_student + t_opt
        print(f"   iteration {it}: sampling {t_samp:8.1f} ms ({t_samp / it:6.2f} per step)  frozen fwd {t_frozen:7.1f}  student "
              f"fwd+head+bwd {t_student:7.1f}  optimiser+refresh {t_opt:6.2f}  sum {total:8.1f} ms", flush=True)
        np.random.seed(0)
        torch.manual_seed(0)
        gen = E.draws(1, tr.nsteps)
        draws = [next(gen) for _ in range(args.draws)]
        pairs = [["concept", "concept"]]
        tr.iteration(pairs, draws[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d in draws:
            loss = tr.iteration(pairs, d)
        torch.cuda.synchronize()
        mean = (time.perf_counter() - t0) / len(draws) * 1e3
        mean_it = sum(d[1] for d in draws) / len(draws)
        print(f"   {len(draws)} seeded draws (mean iteration {mean_it:.1f}, concept == erase_from: 2 frozen rows): {mean:8.1f} ms per "
              f"iteration, last loss {float(loss.item()):.4e}; 1000 iterations: {mean:6.1f} s = {mean / 60:.1f} min", flush=True)
        if method == args.methods.split(",")[0]:
            for rnd in range(3):
                tc = ms(lambda: tr.sample(emb["concept"], emb[""], lat, it), 1)
                tr.graph = False
                te = ms(lambda: tr.sample(emb["concept"], emb[""], lat, it), 1)
                tr.graph = True
                print(f"   sampling {it} steps, round {rnd}: captured {tc:8.1f} ms  eager {te:8.1f} ms  ({te / tc:4.2f} x)", flush=True)
        # the optimiser kernel alone: the table against one contiguous range of the same element count
        s, o = student.store, tr.opt
        w = s.w if dtype == torch.bfloat16 else None
        nb = n_tr * (34 if w is not None else 32)
        t_seg = ms(lambda: k.adamw_segments(s.master, s.grad, o.m, o.v, o.table, o.lr_dev, 0.9, 0.999, 1e-8, 0.0, o.bc_dev, 1.0,
                                            True, w_bf16=w), 10) * 1e3
        t_one = ms(lambda: k.adamw(s.master[:n_tr], s.grad[:n_tr], o.m, o.v, n_tr, o.lr_dev, 0.9, 0.999, 1e-8, 0.0, o.bc_dev, 1.0,
                                   True, w_bf16=None if w is None else w[:n_tr]), 10) * 1e3
        print(f"   pdmk_adamw_segments {t_seg:8.1f} us ({nb / t_seg / 1e6:5.2f} TB/s)   pdmk_adamw contiguous {t_one:8.1f} us "
              f"({nb / t_one / 1e6:5.2f} TB/s)", flush=True)
        s.refresh()
        del tr
    del frozen, student, pipe, vae
    torch.cuda.empty_cache()
