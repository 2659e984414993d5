"""ESD's oracle for tests/test_esd_gpu.py: the reference's iteration restated on the CPU oracle U-Net
(pdm_ref.unet.unet_forward) with autograd and torch.optim.Adam over the trained subset, fp32."""
import os

import torch


def oracle_model(tree):
    """(oracle config, pruning info, fp32 state dict) of data_fixtures.write_pruned_checkpoint_tree's checkpoint."""
    from pdm_ref import weights as oweights
    from pdm_ref.config import UNetConfig as OCfg
    ocfg = OCfg.tiny()
    av = torch.load(os.path.join(tree["ck"], "arch_vector.pt"), map_location="cpu")
    _, info = oweights.prune_state_dict(oweights.init_dense_state_dict(ocfg, seed=0), ocfg, av)
    return ocfg, info, {n: t.clone() for n, t in tree["sd"].items()}


def inputs(hw=16, T=13, ctx=64, seed=43):
    """x [1, 4, hw, hw] and three embeddings of std 1 (so that e_p - e_n is no difference of near-equal numbers)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, hw, hw, generator=g)
    emb_p, emb_n, emb_f = (torch.randn(1, T, ctx, generator=g) for _ in range(3))
    return x, emb_p, emb_n, emb_f


def predictions(frozen, ocfg, info, x, t, emb_p, emb_n, emb_f, same):
    from pdm_ref import unet as ounet
    tt = torch.tensor([int(t)])
    with torch.no_grad():
        e_p = ounet.unet_forward(frozen, ocfg, info, x, tt, emb_p)
        e_n = ounet.unet_forward(frozen, ocfg, info, x, tt, emb_n)
        e_f = e_n.clone() if same else ounet.unet_forward(frozen, ocfg, info, x, tt, emb_f)
    return e_p, e_n, e_f


def esd_loss(P, frozen, ocfg, info, x, t, emb_p, emb_n, emb_f, same, ng):
    """esd_diffusers.py:90-105 (guidance_scale 1: the text row).  Returns (loss with graph, (e_p, e_n, e_f))."""
    from pdm_ref import unet as ounet
    e_p, e_n, e_f = predictions(frozen, ocfg, info, x, t, emb_p, emb_n, emb_f, same)
    e_s = ounet.unet_forward(P, ocfg, info, x, torch.tensor([int(t)]), emb_f)
    return torch.nn.functional.mse_loss(e_s, e_f - (ng * (e_p - e_n))), (e_p, e_n, e_f)


def partial_sampling(P, ocfg, info, sch, latents, emb_p, emb_n, nsteps, end_iteration, guidance=3.0):
    """`end_iteration` DDIM steps (eta 0) of the nsteps-step schedule at `guidance`; the coefficients are the host-side
    float64 ones of DDIMScheduler.coefficients."""
    from pdm_ref import unet as ounet
    sch.set_timesteps(nsteps)
    ehs = torch.cat([emb_n, emb_p])
    with torch.no_grad():
        for t in sch.timesteps.tolist()[:end_iteration]:
            out = ounet.unet_forward(P, ocfg, info, torch.cat([latents] * 2), torch.full((2,), t, dtype=torch.long), ehs)
            un, tx = out.chunk(2)
            c_x, c_m = sch.coefficients(int(t))
            latents = c_x * latents + c_m * (un + guidance * (tx - un))
    return latents
