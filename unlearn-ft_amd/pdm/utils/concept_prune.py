"""ConceptPrune on the pruned student (the reference's baselines/concept_prune/wanda.py, save_union_over_time.py and the parts
of utils/base_utils.py they use): Wanda scores |W| * ||activation|| of the second feed-forward Linear of every transformer block
(`...ff.net.2`), per denoising step, for a set of base prompts and the same prompts with the concept; a weight is "skilled" at a
step when it is among the top skill_ratio of its row for the concept prompts and scores higher there than for the base prompts;
weights that are skilled at more than select_ratio * T steps are zeroed.  No training.

Host side (no GPU needed): the prompt builders, the result path rules, k / threshold arithmetic, the checkpoint format.
GPU side: `WandaObserver` (pdmk_rownorm_colsq on the GEGLU output the engine hands over: nothing is copied to the host while
sampling), `union_counts` (pdmk_wanda_count, one launch per layer for all T) and `apply_counts` (pdmk_wanda_apply).

Only hook_module `unet` is built.  The reference's per-timestep pickles of selected neurons (an intermediate that only its
remove_neurons.py reads) are not written: the counts over time are formed on the device in one pass.

Neuron removal at sampling time (the reference's remove_neurons.py with neuron_receivers/neuron_remover.py: at U-Net call t
layer l runs with W * (1 - mask[t][l])) is `TimestepMasks`: the same selection as one bit per (t, o, f) on the device
(pdmk_wanda_select), applied to the engine's compute weights by one launch per U-Net call (pdmk_masked_weights), in the eager
sampler and as the first node of the captured one (`StableDiffusionPruningPipeline(..., neuron_masks=)`).
"""
import os
from types import SimpleNamespace

import torch

from .load_models import golden_path

HOOK_MODULES = ("unet",)
HOOK_MODULES_NOT_BUILT = ("text", "unet-ffn-1", "attn_key", "attn_val")
ART_TARGETS = ("painting", "Van Gogh", "Monet", "Pablo Picasso", "Salvador Dali", "Leonardo Da Vinci")
OBJECT_TARGETS = ("cassette player", "chain saw", "church", "gas pump", "tench", "garbage truck", "english springer",
                  "golf ball", "parachute", "french horn")
GENDER_TARGETS = ("female", "male")
MEMORIZE_PREFIXES = ("memorize", "coco_memorize", "tv_memorize", "mv_memorize", "cluster")
GUIDANCE = 7.5
SAVED_PAIRS = 5


# ---- flags, target types and prompts
def check_hook_module(hook_module):
    if hook_module in HOOK_MODULES_NOT_BUILT:
        raise NotImplementedError(f"--hook_module {hook_module}: not built here (built: {', '.join(HOOK_MODULES)})")
    if hook_module not in HOOK_MODULES:
        raise ValueError(f"--hook_module {hook_module!r}: expected one of {', '.join(HOOK_MODULES + HOOK_MODULES_NOT_BUILT)}")


def target_type(target):
    """`art` or `naked`; the object, gender and memorize types (their word lists are not data files) raise."""
    if target in ART_TARGETS:
        return "art"
    if target == "naked":
        return "naked"
    for kind, names in (("object", OBJECT_TARGETS), ("gender", GENDER_TARGETS)):
        if target in names:
            raise NotImplementedError(f"--target {target}: target type `{kind}` is not built here (built: art, naked)")
    if target.startswith(MEMORIZE_PREFIXES):
        raise NotImplementedError(f"--target {target}: target type `memorize` is not built here (built: art, naked)")
    raise ValueError(f"--target {target!r}: expected one of {', '.join(ART_TARGETS + ('naked',))}")


def default_words_dir():
    return golden_path("concept_prune")


def read_words(path):
    """One word (or phrase) per line, surrounding blanks removed, empty lines skipped, in file order."""
    with open(path, encoding="utf-8") as f:
        words = [line.strip() for line in f]
    words = [w for w in words if w]
    if not words:
        raise ValueError(f"{path}: no words")
    return words


def build_prompts(target, base="things", words_dir=None):
    """(base prompts, target prompts), pair i from word i.  art: `a photo of a {thing}` / `a {thing} in the style of {target}`
    over <base>.txt; naked: `a photo of a {thing}` / `a photo of a {target} {thing}` over humans.txt."""
    kind = target_type(target)
    words_dir = words_dir or default_words_dir()
    words = read_words(os.path.join(words_dir, ("humans" if kind == "naked" else base) + ".txt"))
    base_prompts = [f"a photo of a {w}" for w in words]
    if kind == "art":
        return base_prompts, [f"a {w} in the style of {target}" for w in words]
    return base_prompts, [f"a photo of a {target} {w}" for w in words]


# ---- paths (Config.configure)
def result_paths(args):
    """results/results_seed_<seed>/<res_path.split('/')[1]>/<model>/<target>/ with images/, skilled_neurons/<skill_ratio>/ and
    checkpoints/ below it; --result_dir replaces the first three components."""
    from .erasure_utils import model_component
    check_hook_module(args.hook_module)
    root = args.result_dir or f"results/results_seed_{args.seed}/" + args.res_path.split("/")[1]
    res = os.path.join(root, model_component(args.model_id), args.target)
    return SimpleNamespace(res_path=res, images=os.path.join(res, "images"),
                           skilled_neurons=os.path.join(res, "skilled_neurons", str(args.skill_ratio)),
                           after_removal_results=os.path.join(res, "after_removal_results", str(args.skill_ratio)),
                           checkpoints=os.path.join(res, "checkpoints"))


def checkpoint_name(skill_ratio, timesteps, select_ratio):
    return f"skill_ratio_{skill_ratio}_timesteps_{timesteps}_threshold{select_ratio}.pt"


def top_k(skill_ratio, width):
    return int(skill_ratio * width)


def count_threshold(select_ratio, timesteps):
    """mask = count > select_ratio * T, compared as floats."""
    return float(select_ratio * timesteps)


def default_config_path():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "configs", "baselines",
                        "concept_prune_wanda.yaml")


def add_arguments(parser):
    """The reference's flags (None = the value of the settings YAML) and this build's additions."""
    for name, typ in (("gpu", int), ("dbg", bool), ("target", str), ("base", str), ("model_id", str), ("skill_ratio", float),
                      ("timesteps", int), ("select_ratio", float), ("hook_module", str), ("base_config_path", str),
                      ("ckpt_path", str)):
        parser.add_argument("--" + name, type=typ, default=None)
    parser.add_argument("--seed", type=int, default=None)
    parser.add_argument("--result_dir", type=str, default=None, help="replaces results/results_seed_<seed>/<res_path part>")
    parser.add_argument("--mixed_precision", type=str, default=None, choices=["no", "bf16"])
    parser.add_argument("--scheduler", type=str, default="ddim", choices=["ddim", "pndm"])
    parser.add_argument("--settings", type=str, default=None, help="settings YAML (default: configs/baselines/concept_prune_wanda.yaml)")
    parser.add_argument("--words_dir", type=str, default=None, help="word lists (default: tests/golden/concept_prune)")
    parser.add_argument("--image_resolution", type=int, default=768, help="when <model_id>/unet/config.json is absent")
    parser.add_argument("--tiny", action="store_true", help="tiny U-Net topology (tests)")
    return parser


def resolve_args(args):
    """Flags left at None take the settings YAML's value (the reference: wanda_config.yaml updated by the command line)."""
    import yaml
    with open(args.settings or default_config_path()) as f:
        settings = yaml.safe_load(f)
    for key, value in settings.items():
        if getattr(args, key, None) is None:
            setattr(args, key, value)
    if args.target is None or args.ckpt_path is None:
        raise ValueError("--target and --ckpt_path are required")
    check_hook_module(args.hook_module)
    target_type(args.target)
    return args


# ---- the layers
def ffn_layers(unet):
    """[(key `...ff.net.2`, rows O, width F, padded width)] of the student's feed-forward blocks in execution order (down, mid,
    up) - the alphabetical order of the key names."""
    out = []
    for name in unet.engine.ffn_index:
        key = name + ".transformer_blocks.0.ff.net.2"
        e = unet.store.by_key[key + ".weight"]
        out.append((key, e.logical[0], e.logical[1], e.shape[1]))
    return out


class WandaObserver:
    """acc[t][l][f] += sum_m (G[m, f] / max(||G[m, :]||, 1e-12))^2 for the GEGLU output G that feeds layer l's ff.net.2 at U-Net
    call t of a sampling run: one flat fp32 arena [T][sum of the padded widths], filled by pdmk_rownorm_colsq from the tensor
    the engine hands over.  Slot t is the U-Net call number since reset_time_layer(); with repeat_first (PNDM: N + 1 calls for N
    steps, the first timestep twice) calls 0 and 1 both add to slot 0."""

    def __init__(self, unet, timesteps, repeat_first=False):
        self.layers = ffn_layers(unet)
        self.T, self.L, self.repeat_first = int(timesteps), len(self.layers), bool(repeat_first)
        self.offsets, off = [], 0
        for _key, _o, _f, fp in self.layers:
            self.offsets.append(off)
            off += fp
        self.width = off
        self.arena = torch.zeros(self.T * self.width, device=unet.device, dtype=torch.float32)
        self.call = self.layer = 0

    def reset_time_layer(self):
        self.call = self.layer = 0

    def slot(self):
        return max(self.call - 1, 0) if self.repeat_first else self.call

    def __call__(self, layer, gl):
        from .. import _pdmk as k
        if layer != self.layer:
            raise RuntimeError(f"WandaObserver: layer {layer} called, {self.layer} expected")
        t, fp = self.slot(), self.layers[layer][3]
        if t >= self.T:
            raise RuntimeError(f"WandaObserver: U-Net call {self.call} of a run, but only {self.T} timestep slots "
                               f"(reset_time_layer() starts a run)")
        if gl.shape[1] != fp:
            raise RuntimeError(f"WandaObserver: layer {layer} is {gl.shape[1]} wide, {fp} expected")
        at = t * self.width + self.offsets[layer]
        k.rownorm_colsq(gl, self.arena[at:at + fp])
        self.layer += 1
        if self.layer == self.L:
            self.layer, self.call = 0, self.call + 1

    def norms(self):
        """[fp32 [T, F_l] on the device]: sqrt of the accumulators, the padding columns cut off."""
        a = self.arena.view(self.T, self.width)
        return [a[:, off:off + f].sqrt().contiguous() for off, (_k, _o, f, _fp) in zip(self.offsets, self.layers)]

    def save(self, path):
        """The reference's format: {t: {l: tensor[F]}} of norms (CPU fp32)."""
        n = [x.cpu() for x in self.norms()]
        torch.save({t: {l: n[l][t].clone() for l in range(self.L)} for t in range(self.T)}, path)


def load_norms(path, device=None):
    """[fp32 [T, F_l]] from a {t: {l: tensor[F]}} file."""
    d = torch.load(path, map_location="cpu")
    T, L = len(d), len(d[0])
    out = [torch.stack([d[t][l].to(torch.float32).reshape(-1) for t in range(T)]).contiguous() for l in range(L)]
    return [x.to(device) for x in out] if device is not None else out


class observing:
    """with observing(unet, observer): the engine calls `observer` (the sampler then takes its eager loop)."""

    def __init__(self, unet, observer):
        self.engine, self.observer = unet.engine, observer

    def __enter__(self):
        self.before, self.engine.ffn_observer = self.engine.ffn_observer, self.observer
        return self.observer

    def __exit__(self, *exc):
        self.engine.ffn_observer = self.before


# ---- observation (GPU)
@torch.no_grad()
def observe(pipe, obs_base, obs_target, base_prompts, target_prompts, seed, steps, resolution, images_dir=None):
    """One image per prompt of every pair from the same seed (guidance 7.5, the doubled batch), the base prompt's activations
    into obs_base and the target prompt's into obs_target; the first five pairs are saved as base_{i}.jpg / target_{i}.jpg."""
    from PIL import Image
    dev = pipe.device
    for i, (pb, pt) in enumerate(zip(base_prompts, target_prompts)):
        print("text: ", pb, pt)
        for name, prompt, obs in (("base", pb, obs_base), ("target", pt, obs_target)):
            obs.reset_time_layer()
            gen = torch.Generator(device=dev).manual_seed(int(seed))
            with observing(pipe.unet, obs):
                img = pipe(prompt=[prompt], num_inference_steps=steps, guidance_scale=GUIDANCE, generator=gen, height=resolution,
                           width=resolution, output_type="u8_round").images[0]
            if images_dir is not None and i < SAVED_PAIRS:
                Image.fromarray(img).save(os.path.join(images_dir, f"{name}_{i}.jpg"))


# ---- scores, union over time, mask (GPU)
def _weight_view(unet, key):
    e = unet.store.by_key[key + ".weight"]
    return unet.store.p(key + ".weight").view(e.shape), e


@torch.no_grad()
def union_counts(unet, base_norms, target_norms, skill_ratio):
    """{layer key: int32 [O, F] (CPU)}: at how many timesteps each weight of ff.net.2 is skilled (module docstring)."""
    from .. import _pdmk as k
    layers = ffn_layers(unet)
    if len(base_norms) != len(layers) or len(target_norms) != len(layers):
        raise ValueError(f"norms of {len(base_norms)} / {len(target_norms)} layers, the model has {len(layers)}")
    out = {}
    for (key, O, F, _fp), nb, nt in zip(layers, base_norms, target_norms):
        w, e = _weight_view(unet, key)
        nb = nb.to(unet.device, torch.float32).contiguous()
        nt = nt.to(unet.device, torch.float32).contiguous()
        count = torch.zeros((O, F), device=unet.device, dtype=torch.int32)
        k.wanda_count(w, nb, nt, top_k(skill_ratio, F), count, O=O, F=F, ldw=e.shape[1])
        out[key] = count.cpu()
    return out


@torch.no_grad()
def apply_counts(unet, counts, select_ratio, timesteps):
    """W <- W * (1 - (count > select_ratio * T)) on the fp32 master weights (the compute copies are refreshed); returns
    {layer key: share of masked weights}."""
    from .. import _pdmk as k
    thr = count_threshold(select_ratio, timesteps)
    density = {}
    for key, O, F, _fp in ffn_layers(unet):
        c = counts[key].to(unet.device, torch.int32).contiguous()
        w, e = _weight_view(unet, key)
        k.wanda_apply(w, c, thr, O=O, F=F, ldw=e.shape[1])
        density[key] = float((c.to(torch.float32) > thr).float().mean().item())
    unet.store.refresh()
    return density


# ---- per-timestep masks: neuron removal while sampling (the reference's remove_neurons.py / NeuronRemover)
def call_slot(call, repeat_first=False):
    """The timestep slot of U-Net call `call` of a sampling run (WandaObserver.slot): the call number, or with repeat_first
    (PNDM: the first timestep is called twice) 0, 0, 1, 2, ..."""
    return max(int(call) - 1, 0) if repeat_first else int(call)


def pack_bits(mask):
    """bool [..., F] -> int32 [..., (F + 31) // 32]: bit f & 31 of word f >> 5 (include/pdmk.h pdmk_wanda_select); the bits
    past F in the last word are 0."""
    F = mask.shape[-1]
    rw = (F + 31) // 32
    m = torch.zeros(tuple(mask.shape[:-1]) + (rw * 32,), dtype=torch.int64, device=mask.device)
    m[..., :F] = mask.to(torch.int64)
    words = (m.view(tuple(mask.shape[:-1]) + (rw, 32)) << torch.arange(32, device=mask.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def unpack_bits(words, F):
    """int32 [..., (F + 31) // 32] -> bool [..., F], the inverse of pack_bits."""
    rw = (F + 31) // 32
    if words.shape[-1] != rw:
        raise ValueError(f"unpack_bits: {words.shape[-1]} words per row, F = {F} takes {rw}")
    w = words.to(torch.int64) & 0xFFFFFFFF
    bits = (w[..., None] >> torch.arange(32, device=words.device)) & 1
    return bits.reshape(tuple(words.shape[:-1]) + (rw * 32,))[..., :F].to(torch.bool)


class TimestepMasks:
    """mask[t][l] of every `...ff.net.2` of `unet` as bits on the device - one arena int32 [T][sum_l O_l * row_words_l], layer
    after layer in ffn_layers() order - and what applies them while sampling: at U-Net call t the engine's compute weights of
    those layers are `pristine * (1 - mask[slot(t)])`, set by ONE pdmk_masked_weights launch from a pristine copy of the
    layers' weights (in fp32 the compute arena IS the master arena: masking in place would lose the weights).

        masks = TimestepMasks.from_norms(unet, base_norms, target_norms, skill_ratio)
        with masks.attach():                      # the pristine copy is taken; restored on exit, on an error too
            masks.apply(slot=3)                   # or apply(state=device call counter, repeat_first=...)

    The pristine buffer, the bit arena and the table are allocated once and keep their addresses, so a captured graph that
    holds the launch stays valid from one attach() to the next.  A new object starts with all-zero masks."""

    def __init__(self, unet, timesteps):
        from .. import _pdmk as k
        self.unet, self.T = unet, int(timesteps)
        if self.T < 1:
            raise ValueError(f"TimestepMasks: {timesteps} timesteps")
        self.layers = ffn_layers(unet)
        st = unet.store
        self.table = k.MaskTable([(st.by_key[key + ".weight"].off, O, F, fp) for key, O, F, fp in self.layers], unet.device)
        self.bits = torch.zeros((self.T, self.table.words), device=unet.device, dtype=torch.int32)
        self._src = torch.zeros(self.table.src_elems, device=unet.device, dtype=st.w.dtype)
        self.attached = False

    def layer_bits(self, l):
        """int32 [T, O, row_words] view of layer l's words."""
        _d, _s, boff, O, F, _ld = self.table.layers[l]
        rw = (F + 31) // 32
        return self.bits[:, boff:boff + O * rw].view(self.T, O, rw)

    @classmethod
    @torch.no_grad()
    def from_norms(cls, unet, base_norms, target_norms, skill_ratio):
        """The masks of pdmk_wanda_count's selection (on the fp32 master weights, as union_counts), one pdmk_wanda_select per
        layer for all T; base_norms / target_norms: [fp32 [T, F_l]] as load_norms() / WandaObserver.norms() give them."""
        from .. import _pdmk as k
        layers = ffn_layers(unet)
        if len(base_norms) != len(layers) or len(target_norms) != len(layers):
            raise ValueError(f"norms of {len(base_norms)} / {len(target_norms)} layers, the model has {len(layers)}")
        self = cls(unet, base_norms[0].shape[0])
        for l, ((key, O, F, _fp), nb, nt) in enumerate(zip(layers, base_norms, target_norms)):
            if tuple(nb.shape) != (self.T, F) or tuple(nt.shape) != (self.T, F):
                raise ValueError(f"{key}: norms {tuple(nb.shape)} / {tuple(nt.shape)}, expected {(self.T, F)}")
            w, e = _weight_view(unet, key)
            boff = self.table.layers[l][2]
            k.wanda_select(w, nb.to(unet.device, torch.float32).contiguous(), nt.to(unet.device, torch.float32).contiguous(),
                           top_k(skill_ratio, F), self.bits[:, boff:boff + O * ((F + 31) // 32)], O=O, F=F, ldw=e.shape[1])
        return self

    def density(self):
        """{layer key: [T floats]}: the share of masked weights of the layer at every timestep."""
        out = {}
        for l, (key, O, F, _fp) in enumerate(self.layers):
            n = unpack_bits(self.layer_bits(l), F).sum((1, 2)).tolist()
            out[key] = [c / (O * F) for c in n]
        return out

    @torch.no_grad()
    def attach(self):
        """Takes the pristine copy of the layers' compute weights (a second attach() without detach() keeps the first copy)."""
        if not self.attached:
            w = self.unet.store.w
            for d, s, _b, O, _F, ld in self.table.layers:
                self._src[s:s + O * ld].copy_(w[d:d + O * ld])
            self.attached = True
        return self

    @torch.no_grad()
    def detach(self):
        """Writes the pristine weights back: the arena is then bit for bit what attach() found."""
        if self.attached:
            from .. import _pdmk as k
            k.masked_weights(self.unet.store.w, self._src, self.table)
            self.attached = False

    def __enter__(self):
        return self.attach()

    def __exit__(self, *exc):
        self.detach()

    def apply(self, slot=None, state=None, repeat_first=False):
        """The compute weights of timestep slot `slot` (a host int; outside [0, T): unmasked), or of the U-Net call number in
        the int32 device tensor `state`[0], which repeat_first maps as call_slot() does."""
        from .. import _pdmk as k
        if not self.attached:
            raise RuntimeError("TimestepMasks.apply: attach() first (the pristine copy is what the masked weights are made from)")
        if (slot is None) == (state is None):
            raise ValueError("TimestepMasks.apply: pass slot= or state=")
        k.masked_weights(self.unet.store.w, self._src, self.table, self.bits, slot=-1 if slot is None else int(slot),
                         state=state, repeat_first=repeat_first)


def masked_state_dict(unet):
    """The full state dict under the reference's key names; the masked layers' weights as fp16 (kept values rounded through
    fp16), every other tensor as the model holds it."""
    sd = unet.state_dict()
    for key, _o, _f, _fp in ffn_layers(unet):
        sd[key + ".weight"] = sd[key + ".weight"].to(torch.float16)
    return sd
