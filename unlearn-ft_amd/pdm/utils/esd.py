"""ESD (the reference's baselines/erasing/esd_diffusers.py and utils/utils.py), host side: which concepts are erased from
which, the checkpoint's name and nesting, which modules `--train_method` trains and where they lie in the parameter arena,
and the three host draws of an iteration.  Nothing here needs a GPU; the training loop is pdm/training/esd.py.
"""
import os

import numpy as np
import torch

NSTEPS = 50                      # esd_diffusers.py:24
GUIDANCE = 3.0                   # esd_diffusers.py:82
TRAIN_METHODS = ("xattn", "noxattn", "selfattn")


# ---- concepts (esd_diffusers.py:35-53, :144-147)
def build_pairs(erase_concept, erase_from=None):
    """[[concept, erase_from]] from the two comma-separated flags; a single erase_from serves every concept, any other length
    mismatch raises; erase_from None is the concept string itself (esd_diffusers.py:138-139)."""
    if erase_from is None:
        erase_from = erase_concept
    concepts = [a.strip() for a in erase_concept.split(",")]
    froms = [a.strip() for a in erase_from.split(",")]
    if len(froms) != len(concepts):
        if len(froms) != 1:
            raise Exception("Erase from concepts length need to match erase concepts length")
        froms = [froms[0] for _ in concepts]
    return [[e, f] for e, f in zip(concepts, froms)]


def _squash(s):
    return s.lower().replace(" ", "").replace(",", "")


def checkpoint_name(erase_concept, erase_from, train_method, negative_guidance, iterations):
    if erase_from is None:
        erase_from = erase_concept
    return (f"esd-{_squash(erase_concept)}_from_{_squash(erase_from)}-{train_method}_{negative_guidance}"
            f"-epochs_{iterations}")


def checkpoint_path(save_path, *name_args):
    return f"{save_path}/{checkpoint_name(*name_args)}.pt"


# ---- trainable modules (utils.py:359-403)
def _selected(module, train_method):
    if train_method == "xattn":
        return "attn2" in module
    if train_method == "xattn-strict":        # utils.py:382 skips unless the name holds attn2, to_q AND to_k: no module does
        return "attn2" in module and "to_q" in module and "to_k" in module
    if train_method == "noxattn":
        return "attn2" not in module
    if train_method == "selfattn":
        return "attn1" in module
    raise NotImplementedError(f"train_method: {train_method} is not implemented.")


def check_train_method(train_method):
    """What the reference does with the flag before the first iteration: an unknown method raises NotImplementedError at the
    first Linear, `xattn-strict` selects nothing and torch.optim.Adam refuses the empty list."""
    _selected("", train_method)
    if train_method == "xattn-strict":
        raise ValueError("optimizer got an empty parameter list")


def trainable_names(names, kinds, train_method):
    """The state-dict names ESD trains.  names: diffusers parameter names (no `unet.` prefix); kinds: for each of them the
    kind of the arena entry that holds it ("conv3" / "lin" / "vec").  A module is a Linear or Conv2d when its weight lies in
    a conv3 / lin entry (norm affines are vec); its bias follows it."""
    check_train_method(train_method)
    modules = {n[:-len(".weight")] for n, kd in zip(names, kinds) if kd in ("conv3", "lin") and n.endswith(".weight")}
    out = []
    for n in names:
        module = n.rsplit(".", 1)[0]
        if module in modules and _selected("unet." + module, train_method):
            out.append(n)
    if not out:
        raise ValueError("optimizer got an empty parameter list")
    return out


def entry_names(entries):
    """(names, kinds) of a list of params.Entry, every source name once."""
    seen = {}
    for e in entries:
        for src in e.srcs:
            seen.setdefault(src[0], e.kind)
    return list(seen), list(seen.values())


def trainable_entries(entries, train_method):
    """The arena entries ESD trains, in arena order.  Every entry lies wholly inside or wholly outside the set (the fused
    entries hold only attn2, only attn1 or only non-attn2 Linears); one that does not raises."""
    names, kinds = entry_names(entries)
    chosen = set(trainable_names(names, kinds, train_method))
    out = []
    for e in entries:
        inside = [src[0] in chosen for src in e.srcs]
        if any(inside) != all(inside):
            raise ValueError(f"{e.key}: only some of its tensors are trained by {train_method}")
        if inside[0]:
            out.append(e)
    return out


def segments(entries):
    """[(offset, length)] of the entries' 128-element slots, neighbours merged, sorted by offset."""
    out = []
    for e in sorted(entries, key=lambda e: e.off):
        n = (e.numel + 127) // 128 * 128
        if out and out[-1][0] + out[-1][1] == e.off:
            out[-1] = (out[-1][0], out[-1][1] + n)
        else:
            out.append((e.off, n))
    return out


# ---- the draws of an iteration (esd_diffusers.py:61, :72, :74)
def draws(n_pairs, nsteps=NSTEPS, latent_shape=(1, 4, 64, 64)):
    """Yields (pair index, iteration, initial latents) forever, making exactly the reference's three host calls in its order
    on the global numpy and torch CPU generators."""
    while True:
        index = int(np.random.choice(n_pairs, 1, replace=False)[0])
        iteration = torch.randint(1, nsteps - 1, (1,)).item()
        latents = torch.randn(latent_shape)
        yield index, iteration, latents


def timestep_index(iteration, nsteps=NSTEPS, train_steps=1000):
    """Index into the 1000-step schedule of the frozen / trained predictions (esd_diffusers.py:88)."""
    return int(iteration / nsteps * train_steps)


def prediction_timestep(scheduler, iteration, nsteps=NSTEPS):
    """The U-Net timestep of the predictions: `scheduler.timesteps[timestep_index]` of the 1000-step schedule.  Leaves the
    scheduler set to `nsteps` steps."""
    train_steps = scheduler.config.num_train_timesteps
    scheduler.set_timesteps(train_steps)
    t = int(scheduler.timesteps[timestep_index(iteration, nsteps, train_steps)])
    scheduler.set_timesteps(nsteps)
    return t


# ---- checkpoint (utils.py:440-444; read by erasure_utils.esd_state_dict)
def nest_state_dict(flat, prefix="unet."):
    """{"<module>.weight": w, "<module>.bias": b} -> {"unet.<module>": {"weight": w, "bias": b}}, in the given order."""
    nested = {}
    for name, t in flat.items():
        module, leaf = name.rsplit(".", 1)
        nested.setdefault(prefix + module, {})[leaf] = t
    return nested


def unnest_state_dict(nested):
    """The inverse, as the evaluation scripts read the file (erasure_utils.esd_state_dict)."""
    from .erasure_utils import esd_state_dict
    return esd_state_dict(nested)


def save_checkpoint(path, flat):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    torch.save(nest_state_dict({n: t.detach().to(torch.float32).cpu().contiguous() for n, t in flat.items()}), path)
    return path
