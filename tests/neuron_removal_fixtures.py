"""Inputs and CPU oracles of the neuron-removal tests (tests/test_neuron_removal_gpu.py, tests/test_neuron_removal_host.py): the
bit layout of pdmk_wanda_select written as a Python loop, arenas for pdmk_masked_weights, and the tiny pipeline of
tests/test_concept_prune_gpu.py::_pipe restated.  The selection oracle is concept_prune_fixtures.count_oracle."""
import torch

import concept_prune_fixtures as fx

# (O, F, ld) of the layers of the pdmk_masked_weights arena: one 16-byte chunk per row, padded rows, and a layer that is cut
# into several workgroups (2568 columns: 6 rows per MASK_PIECE)
MASK_LAYERS = [(5, 8, 8), (40, 72, 96), (17, 2568, 2568)]
MASK_T = 3
PAD_VALUE = 1e4


# ---- the bit layout
def pack_loop(mask):
    """bool [R, F] -> int32 [R, (F + 31) // 32], bit by bit: bit f & 31 of word f >> 5."""
    R, Fd = mask.shape
    rw = (Fd + 31) // 32
    rows = []
    for r in range(R):
        words = [0] * rw
        for f in range(Fd):
            if bool(mask[r, f]):
                words[f >> 5] |= 1 << (f & 31)
        rows.append([w - (1 << 32) if w >= (1 << 31) else w for w in words])
    return torch.tensor(rows, dtype=torch.int32).reshape(R, rw)


def unpack_loop(words, Fd):
    """int32 [R, rw] -> bool [R, F], bit by bit."""
    R = words.shape[0]
    out = torch.zeros((R, Fd), dtype=torch.bool)
    for r in range(R):
        for f in range(Fd):
            out[r, f] = bool((int(words[r, f >> 5]) >> (f & 31)) & 1)
    return out


def selection_oracle(w, nb, nt, k):
    """bool [T, O, F]: count_oracle of every timestep on its own."""
    return torch.stack([fx.count_oracle(w, nb[t:t + 1], nt[t:t + 1], k) for t in range(nt.shape[0])]) > 0


# ---- pdmk_masked_weights
def mask_arena(layers, dtype, seed=0, first=16, gap=40):
    """(arena [n] of `dtype` on the CPU, [(element offset, O, F, ld)]): the layers' weights (never zero) in the F columns,
    PAD_VALUE in the padding columns, in front of the first layer, between the layers and behind the last."""
    g = torch.Generator().manual_seed(seed)
    offs, off = [], first
    for O, Fd, ld in layers:
        offs.append(off)
        off += O * ld + gap
    arena = torch.full((off,), PAD_VALUE, dtype=dtype)
    for o, (O, Fd, ld) in zip(offs, layers):
        w = torch.randn(O, Fd, generator=g)
        w = torch.where(w.abs() < 0.01, torch.ones(()), w).to(dtype)
        arena[o:o + O * ld].view(O, ld)[:, :Fd] = w
    return arena, [(o, O, Fd, ld) for o, (O, Fd, ld) in zip(offs, layers)]


def random_masks(layers, T, seed=1):
    """[bool [T, O, F]] per layer, about a third set."""
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(T, O, Fd, generator=g) < 0.33 for O, Fd, _ld in layers]


def masked_arena(arena, placed, masks, slot):
    """The arena with mask[slot] applied by torch.where (slot None: unchanged)."""
    out = arena.clone()
    if slot is not None:
        for (o, O, Fd, ld), m in zip(placed, masks):
            v = out[o:o + O * ld].view(O, ld)[:, :Fd]
            v.copy_(torch.where(m[slot], torch.zeros((), dtype=arena.dtype), v))
    return out


# ---- the tiny pipeline
def pipe(dev, dtype, scheduler):
    """tests/test_concept_prune_gpu.py::_pipe: the tiny U-Net (dense weights of seed 0, architecture vector of budget 0.6, seed
    1, one depth dropped) and the tiny VAE (seed 7), no text encoder."""
    from pdm_ref import arch as oarch, weights as oweights, vae as ovae
    from pdm_ref.config import UNetConfig as OCfg
    from pdm.models.unet.spec import UNetConfig
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
    from pdm.pipelines.pruning_pipelines import StableDiffusionPruningPipeline
    ocfg, cfg = OCfg.tiny(), UNetConfig.tiny()
    dense = oweights.init_dense_state_dict(ocfg, seed=0)
    av = oarch.random_arch_vector(ocfg, 0.6, seed=1, drop_depth=(1,))
    unet = UNet2DConditionModelPruned(cfg, av, dev, dtype, train=False, init=False)
    unet.load_dense_or_pruned(dense)
    vcfg = ovae.VAEConfig.tiny()
    vae = AutoencoderKL(VAEConfig(block_out_channels=vcfg.block_out_channels, layers_per_block=1), dev, dtype, init=False)
    vae.load_state_dict(ovae.init_state_dict(vcfg, seed=7))
    return StableDiffusionPruningPipeline(vae, None, unet, scheduler)


def sampling_inputs(seed=4):
    """(prompt embeddings, negative embeddings, latents) as test_concept_prune_gpu.py draws them."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 13, 64, generator=g), torch.randn(1, 13, 64, generator=g), torch.randn(1, 4, 16, 16, generator=g)


def norm_sets(layers, T, seed=0):
    """Two seeded norm sets ([fp32 [T, F_l]] each) for the layers [(key, O, F, padded F)] of a U-Net."""
    base, target = [], []
    for l, (_key, _O, Fd, _fp) in enumerate(layers):
        _w, nb, nt = fx.count_inputs(1, Fd, T, seed=seed + l)
        base.append(nb)
        target.append(nt)
    return base, target
