"""UCE debiasing on the pruned student (the reference's baselines/unified-concept-editing/train-scripts/train_debias.py and
eval-scripts/CLIP_classify.py): alternate a measurement - sample images of every concept text, let CLIP say which attribute
text each image is closest to, take the share of images per attribute - with a closed-form edit of every cross-attention
`attn2.to_k` / `attn2.to_v` weight that pushes each concept's projection along the normalised projections of its attribute
texts, by weights the measured shares set, until every share is within 0.05 of uniform.

One old text (a concept in one of five templates) has A new texts (the text with the concept replaced by each attribute).  Per
(old text, projection) block, with O the block's current projection of the old text's window, U_j that of attribute j's window
and Frobenius norms over the block, the reference adds into an alias of O, so the norm is the running one:
    T_0 = O,   T_{j+1} = T_j + (w_j ||T_j||) U_j / ||U_j||,   V = T_A,   D = V - O = sum_j c_j U_j,   c_j = w_j ||T_j|| / ||U_j||.
The edit is progressive (the weights are not reset between iterations; within one, every projection's values come from its
weights at the start):  mat1 = lam W_cur + s_e sum V^T E_old + s_r sum (E_r W_cur^T)^T E_r, mat2 as in pdm/utils/uce.py, hence
    W' = W_cur + s_e D^T Z,     Z = E_old mat2^-1,
the retain terms cancelling as they do there.  mat2 changes only when the retain list does: it is formed, factored and solved
again only then (pdmk_fid_accumulate, pdmk_spd_*, fp64).  O and the U_j of all projections are A + 1 fp32 GEMMs against the master
matrix `attn2_kv_all`, D comes from pdmk_uce_debias_delta (the c_j in fp64 from each block's Gram matrix) and the update is one
more GEMM.  Every text is encoded once per run.

A measurement stays on the device from the latents to the counts: the captured PNDM sampler at the fixed batch `num_images`
(one graph for the run), the VAE decode, pdmk_image_to_u8_ex (numpy_to_pil's rounding), pdmk_image_prep_ex reading those bytes in
place (CLIPProcessor's bicubic resize, centre crop, mean / std), the CLIP image tower through its replay cache and
pdmk_zeroshot_head, which adds each image's mask to an int32 table; one read-back per measurement.

Host side (no GPU needed): `build_texts`, `group_slices`, `schedule`, `read_professions`, the settings of
configs/baselines/uce_debias.yaml and the frame handling of CLIP_classify.py.  GPU side: `classify_frames`, `get_ratios`,
`prepare`, `debias_edit`, `debias_model`, `classify_folder`.

Deviations from the reference: only --base 2.1 (the pruned SD-2.1 student); seeds come from one np.random.RandomState(--seed)
instead of numpy's global state; a zero attribute projection contributes nothing where the reference yields NaN.
"""
import os
import re
from collections import namedtuple

import numpy as np
import torch

from .load_models import golden_path
from .uce import ROW_PAD, _encode, kv_columns

Step = namedtuple("Step", "weights retain_texts bypass done ratios max_change")
Window = namedtuple("Window", "old news old_rows new_rows")


# ---- settings, texts and names (train_debias.py:357-415)
def settings_path():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "configs", "baselines",
                        "uce_debias.yaml")


def load_settings(path=None):
    import yaml
    with open(path or settings_path(), encoding="utf-8") as f:
        return yaml.safe_load(f)


def default_professions_file():
    return golden_path("uce", "professions.txt")


def read_professions(path=None):
    """The unique `profession` values of the reference's data/profession_prompts.csv in order of first appearance, one per line."""
    with open(path or default_professions_file(), encoding="utf-8") as f:
        names = [line.rstrip("\n") for line in f]
    names = [n for n in names if n]
    if not names:
        raise ValueError(f"{path}: no professions")
    return names


def split_list(text):
    return [c.strip() for c in text.split(",")]


def build_texts(concept, attributes, professions=None, base="2.1", settings=None):
    """(old_texts, new_texts, retain_texts, name) by the reference's rules.  `concept`, `attributes`: the comma-separated flag
    strings.  old_texts: five templates per concept; new_texts[i]: old_texts[i] with the concept replaced by each attribute, a
    single attribute twice; retain_texts: `professions` (None: read_professions()) minus those that equal an old text
    case-insensitively; name: the concepts as given, lower-cased and joined by `_` (`default0` stays `default0`),
    `-attributes-`, the attributes with spaces written as 9, `-sd_2_1`."""
    if str(base) != "2.1":
        raise NotImplementedError(f"--base {base}: only 2.1 (the pruned SD-2.1 student) is built here")
    settings = settings or load_settings()
    concepts = split_list(concept)
    name = "_".join(c.lower() for c in concepts)
    if concepts[0] == "default0":
        concepts = [str(c) for c in settings["default0"]]
    attrs = split_list(attributes)
    name += "-attributes-" + "_".join(a.lower().replace(" ", "9") for a in attrs)
    name += f"-sd_{str(base).replace('.', '_')}"
    old_texts, new_texts = [], []
    for c in concepts:
        for template in settings["templates"]:
            text = template.format(concept=c)
            news = [text.replace(c, a) for a in attrs]
            old_texts.append(text)
            new_texts.append(news * 2 if len(news) == 1 else news)
    lower = [t.lower() for t in old_texts]
    professions = read_professions() if professions is None else list(professions)
    retain_texts = [p for p in professions if p.lower() not in lower]
    return old_texts, new_texts, retain_texts, name


def add_arguments(parser):
    """The reference's flags (--base defaults to 2.1 here, the only one built) and this build's additions."""
    parser.add_argument("--concept", help="prompt corresponding to concept to erase", type=str, required=True)
    parser.add_argument("--attributes", help="Attributes to debias", type=str, default="male, female")
    parser.add_argument("--device", help="cuda devices to train on", type=str, default="0")
    parser.add_argument("--base", help="base version for stable diffusion", type=str, default="2.1")
    parser.add_argument("--num_images", help="number of images per concept to generate for validation", type=int, default=10)
    parser.add_argument("--base_config_path", help="Path to base config file", type=str)
    parser.add_argument("--ckpt_path", help="Path to checkpoint file", type=str)
    parser.add_argument("--model_id", type=str, default=None, help="SD-2.1 snapshot directory (tokenizer, text encoder, VAE)")
    parser.add_argument("--clip_model", type=str, default="openai/clip-vit-base-patch32",
                        help="a local transformers CLIP directory or an OpenAI .pt")
    parser.add_argument("--tokenizer", type=str, default=None, help="CLIP tokenizer directory (default: --clip_model's)")
    parser.add_argument("--output_dir", type=str, default=".", help="models/ and info/ are written below it")
    parser.add_argument("--seed", type=int, default=0, help="seed of the np.random.RandomState the sampling seeds come from")
    parser.add_argument("--image_resolution", type=int, default=768, help="when <model_id>/unet/config.json is absent")
    parser.add_argument("--mixed_precision", type=str, default="no", choices=["no", "bf16"])
    parser.add_argument("--tiny", action="store_true", help="tiny U-Net topology (tests)")
    return parser


# ---- slices
def group_slices(n_old, n_new_list, length):
    """((start, stop) of the old text's rows, [(start, stop) of each new text's]) from the attention-mask sums n (BOS + words +
    EOS) of an old text and its A new texts padded to `length` tokens: f = n - 2, far = the largest f of all A + 1, every
    window starts at its own f and has length - far rows.  uce.pair_slices for A new texts."""
    f_old, f_new = n_old - 2, [n - 2 for n in n_new_list]
    far = max(f_new + [f_old])
    return (f_old, length - (far - f_old)), [(f, length - (far - f)) for f in f_new]


# ---- the host step of the outer loop (train_debias.py:229-270)
def schedule(ratios, prev_ratios, prev_max_change, retain_texts, old_texts, max_bias_diff=0.05, weight_step=0.1):
    """One pass of the outer loop's bookkeeping, in fp32 torch on the host as the reference does it, so that every comparison
    falls as it does there.  ratios: one fp32 [A] tensor per old text; an old text whose previous max_change is below
    max_bias_diff was bypassed in the measurement and keeps prev_ratios' entry whatever `ratios` holds for it (None is fine).
    Returns Step(weights, retain_texts, bypass, done, ratios, max_change):
      max_change[c] = max |ratio_c - 1 / A|;  done = max(max_change) < max_bias_diff (then weights is None and the retain
      list is returned as it came);  weights[c] = weight_step (1 / A - ratio_c), times 0 unless max_change[c] > max_bias_diff;
      old texts whose weights[c][0] == 0 join the retain list - a concept whose first share is exactly uniform does, debiased
      or not - and the list then goes through np.unique (sorted, de-duplicated); without one it is left as it is;
      bypass[c] = max_change[c] < max_bias_diff, for the next measurement."""
    ratios = list(ratios)
    if prev_max_change is not None:
        for c, change in enumerate(prev_max_change):
            if change < max_bias_diff:
                ratios[c] = prev_ratios[c]
    ratios = [torch.as_tensor(r, dtype=torch.float32) for r in ratios]
    desired = [torch.ones(len(r)) / len(r) for r in ratios]
    max_change = [(r - d).abs().max() for r, d in zip(ratios, desired)]
    bypass = [bool(c < max_bias_diff) for c in max_change]
    if max(max_change) < max_bias_diff:
        return Step(None, list(retain_texts), bypass, True, ratios, max_change)
    delta = [weight_step * (d - r) for r, d in zip(ratios, desired)]
    delta = [delta[c] if change > max_bias_diff else delta[c] * 0 for c, change in enumerate(max_change)]
    add = [old_texts[c] for c, w in enumerate(delta) if w[0] == 0]
    retain = list(retain_texts)
    if add:
        retain = [str(t) for t in np.unique(retain + add)]
    return Step(delta, retain, bypass, False, ratios, max_change)


# ---- CLIP_classify.py: names and the frame
def sorted_nicely(names):
    """The reference's natural sort: digit runs compare as numbers."""
    def key(name):
        return [int(c) if c.isdigit() else c for c in re.split("([0-9]+)", name)]
    return sorted(names, key=key)


def png_case_number(name):
    """CLIP_classify.py:31: `12_3.png` -> 12."""
    return int(name.split("_")[0].replace(".png", ""))


def bias_columns(attributes):
    return [f"{a.replace(' ', '_')}_bias" for a in attributes]


def write_csv(path, header, rows):
    """DataFrame.to_csv(index=False): floats with repr."""
    import csv
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(list(header))
        for row in rows:
            w.writerow([repr(v) if isinstance(v, float) else v for v in row])
    return path


# ---- measurement (GPU)
_DESC = {}


def frame_descriptors(B, H, W, R, device):
    """(host, device) pdmk_image_desc of B contiguous H x W x 3 frames: short side to R, centre crop - built once per shape."""
    from .data import center_crop_origin, resized_size
    key = (B, H, W, R, str(device))
    if key not in _DESC:
        if (H * W * 3) % 4:
            raise NotImplementedError(f"frames of {H} x {W}: pdmk_image_prep_ex reads every image from a 4-byte word")
        rh, rw = resized_size(H, W, R)
        top, left = center_crop_origin(rh, rw, R)
        d = torch.tensor([[b * H * W * 3, H, W, rh, rw, top, left, 0] for b in range(B)], dtype=torch.int64)
        _DESC[key] = (d, d.to(device))
    return _DESC[key]


def frame_pixels(frames_u8, R):
    """Device uint8 NHWC frames -> CLIP pixel values fp32 [B, 3, R, R]: pdmk_image_prep_ex (Pillow-exact bicubic) reading the
    frames where they lie."""
    from .. import _pdmk as k
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise ValueError("frames: a contiguous uint8 [B, H, W, 3] tensor on the device")
    B, H, W, _ = frames_u8.shape
    desc, desc_dev = frame_descriptors(B, H, W, R, frames_u8.device)
    pix = torch.empty(B, 3, R, R, device=frames_u8.device)
    k.image_prep_ex(frames_u8.view(-1), desc, desc_dev, pix, filter=1)
    return pix


def logit_scale(clip):
    """The host's fp32 exp(logit_scale)."""
    return float(torch.exp(clip.logit_scale.to(torch.float32)))


@torch.no_grad()
def classify_frames(clip, frames_u8, class_features, group=None, hits=None, timing=None):
    """(probs fp32 [B, A], mask int32 [B, A]) of device uint8 NHWC frames against the class-text features [A, D] (as
    encode_text leaves them); hits int32 [G, A] and group int32 [B] (both on the device) as pdmk_zeroshot_head takes them.
    No host copy and, once the tower's graph of this batch size exists, no synchronisation.  timing: a callable(name) called
    after `tower` and `head`."""
    from .. import _pdmk as k
    img = clip.encode_image(frame_pixels(frames_u8, clip.image_size))
    if timing:
        timing("tower")
    out = k.zeroshot_head(img, class_features, logit_scale(clip), group=group, hits=hits)
    if timing:
        timing("head")
    return out


GEMM_BUFFER_LIMIT = 1 << 31          # pdmk_gemm addresses an operand with 32-bit byte offsets


@torch.no_grad()
def decode_frames(pipe, latents):
    """Latents -> device uint8 NHWC frames, the bytes of the pipeline's output_type="u8_round" (diffusers' numpy_to_pil).  One
    decode of the whole batch, as the pipeline's, unless its widest full-resolution map (the VAE's largest channel count, a
    safe over-estimate) would pass the GEMM's 2 GiB operand limit - ten 768 x 768 images do; then the batch is decoded in
    chunks of images, which the VAE treats independently."""
    from .. import _pdmk as k
    vae = pipe.vae
    B, _c, h, w = latents.shape
    f = pipe.vae_scale_factor
    per_image = h * f * w * f * max(vae.cfg.block_out_channels) * (2 if vae.dtype == torch.bfloat16 else 4)
    chunk = max(1, min(B, (GEMM_BUFFER_LIMIT - 1) // per_image))
    u8 = torch.empty((B, h * f, w * f, 3), device=latents.device, dtype=torch.uint8)
    for s in range(0, B, chunk):
        image = vae.decode(latents[s:s + chunk] / vae.cfg.scaling_factor, return_dict=False)[0]
        k.image_to_u8_ex(image.contiguous(), u8[s:s + chunk], 1)
    return u8


def seed_latents(pipe, seed, num_images, resolution):
    """The reference's latents of one seed: one CPU Generator.manual_seed(seed) draws [num_images, C, h, w] in fp32."""
    f = pipe.vae_scale_factor
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randn((num_images, pipe.unet.cfg.in_channels, resolution // f, resolution // f), generator=g, dtype=torch.float32)


@torch.no_grad()
def get_ratios(pipe, clip, tokenizer, old_texts, new_texts, bypass, prev, seeds, num_images, steps, resolution,
               guidance_scale=7.5, timing=None):
    """One fp32 [A] tensor per old text: the share of its len(seeds) x num_images images whose CLIP logit against new text a
    is the row's largest (ties count for each).  bypass[c] true: the text is not sampled and keeps prev[c].  tokenizer: CLIP's.
    Every text is encoded once; sampling runs at the fixed batch num_images; the frames never leave the device; one read-back.
    timing: a callable(name) called after `encode_texts` and after the stages `sample`, `decode`, `tower`, `head` of every
    batch (tools/debias_bench.py)."""
    from .clip_utils import tokenize
    mark = timing or (lambda name: None)
    dev = pipe.device
    n = len(old_texts)
    A = len(new_texts[0])
    if any(len(t) != A for t in new_texts) or len(new_texts) != n:
        raise ValueError("get_ratios: every old text needs the same number of class texts")
    active = [c for c in range(n) if not (bypass is not None and bypass[c])]
    for c in range(n):
        if c not in active:
            print(f"Bypassing Concept {c + 1}")
    hits = torch.zeros((n, A), device=dev, dtype=torch.int32)
    neg = pipe.text_encoder(pipe._tokenize([""]))[0].expand(num_images, -1, -1) if active else None
    embeds = {c: pipe.text_encoder(pipe._tokenize([old_texts[c]]))[0].expand(num_images, -1, -1) for c in active}
    classes = {c: clip.encode_text(tokenize(tokenizer, new_texts[c], context_length=clip.context_length)) for c in active}
    groups = {c: torch.full((num_images,), c, dtype=torch.int32).to(dev) for c in active}
    latents = [seed_latents(pipe, s, num_images, resolution).to(dev) for s in seeds] if active else []
    mark("encode_texts")
    for c in active:
        for lat in latents:
            z = pipe.generate_samples(prompt_embeds=embeds[c], negative_prompt_embeds=neg, latents=lat, num_inference_steps=steps,
                                      guidance_scale=guidance_scale, height=resolution, width=resolution,
                                      output_type="latent").images
            mark("sample")
            frames = decode_frames(pipe, z)
            mark("decode")
            classify_frames(clip, frames, classes[c], groups[c], hits, timing=timing)
    counts = hits.cpu().to(torch.float32)                                 # the measurement's one read-back
    rows = torch.tensor(float(len(seeds) * num_images), dtype=torch.float32)
    return [prev[c] if c not in active else counts[c] / rows for c in range(n)]


# ---- the edit (GPU)
class EditState:
    """What one run keeps between its edits: every text's embedding (encoded once), and of the last edit the stacked windows
    E_old / E_att, the Gram matrix of E_old, the factor of mat2 and Z, with the retain list and scalars they belong to."""

    def __init__(self, text_encoder, tokenizer, device, batch_size=64):
        self.text_encoder, self.tokenizer, self.device, self.batch_size = text_encoder, tokenizer, device, max(int(batch_size), 1)
        self.emb, self.count, self.T = {}, {}, int(tokenizer.model_max_length)
        self.E_old = self.E_att = self.g_old = self.Z = self.row_seg = None
        self.system_key = None
        self.factorisations = 0                      # how often mat2 was formed and factored (tests, tools)

    def encode(self, texts):
        """Encodes those of `texts` that have not been seen yet, in batches."""
        fresh = [t for t in dict.fromkeys(texts) if t not in self.emb]
        for s in range(0, len(fresh), self.batch_size):
            part = fresh[s:s + self.batch_size]
            tok = self.tokenizer(part, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                                 return_tensors="pt")
            y = _encode(self.text_encoder, tok.input_ids, self.device)
            self.emb.update(zip(part, y))
            self.count.update(zip(part, tok.attention_mask.sum(1).tolist()))


@torch.no_grad()
def prepare(text_encoder, tokenizer, old_texts, new_texts, device, batch_size=64):
    """(embeddings, windows) of a run: the EditState with every old and new text encoded, and per old text a Window(old, news,
    old_rows, new_rows) by group_slices."""
    if not old_texts or len(old_texts) != len(new_texts):
        raise ValueError(f"{len(old_texts)} texts to debias, {len(new_texts)} groups of attribute texts")
    A = len(new_texts[0])
    if any(len(n) != A for n in new_texts):
        raise ValueError("every old text needs the same number of attribute texts")
    state = EditState(text_encoder, tokenizer, device, batch_size)
    state.encode(list(old_texts) + [t for news in new_texts for t in news])
    windows = []
    for o, news in zip(old_texts, new_texts):
        a, bs = group_slices(state.count[o], [state.count[t] for t in news], state.T)
        windows.append(Window(o, tuple(news), a, tuple(bs)))
    return state, windows


def _stack_windows(state, windows, K):
    """E_old [mp, K], E_att [A, mp, K] (zero rows from m on) and the first rows of the windows."""
    dev = state.device
    row_seg = [0]
    for w in windows:
        row_seg.append(row_seg[-1] + w.old_rows[1] - w.old_rows[0])
    m, A = row_seg[-1], len(windows[0].news)
    mp = (m + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    E_old = torch.zeros((mp, K), device=dev, dtype=torch.float32)
    E_att = torch.zeros((A, mp, K), device=dev, dtype=torch.float32)
    E_old[:m] = torch.cat([state.emb[w.old][w.old_rows[0]:w.old_rows[1]] for w in windows])
    for j in range(A):
        E_att[j, :m] = torch.cat([state.emb[w.news[j]][w.new_rows[j][0]:w.new_rows[j][1]] for w in windows])
    return E_old, E_att, row_seg


@torch.no_grad()
def debias_edit(unet, embeddings, windows, weights, retain, lamb=0.5, erase_scale=1.0, preserve_scale=0.1, stages=None):
    """One edit of the fp32 master weights of every attn2.to_k / to_v of `unet`, in place, from their current values (module
    docstring), then the compute copies are refreshed.  embeddings, windows: prepare()'s; weights: one fp32 [A] tensor per old
    text; retain: the retained texts (None: ['']).  mat2 is formed, factored and solved for Z only when the retain list or a
    scalar differs from the previous call's; only then is the factorisation's flag read back, and a pivot that is not positive
    raises before any weight is touched.  stages: a callable(name) called after `encode`, `gram_factor`, `solve`, `project`,
    `delta`, `update`."""
    from .. import _pdmk as k
    mark = stages or (lambda name: None)
    st = embeddings
    dev, store = unet.device, unet.store
    if not store.has("attn2_kv_all.weight"):
        raise ValueError("the model has no cross-attention left to edit")
    e = store.by_key["attn2_kv_all.weight"]
    ktot, Kp = e.shape
    K = e.logical[1]
    if K != Kp or K % 16:
        raise NotImplementedError(f"cross_attention_dim {K}: the fp32 GEMM loaders need a multiple of 16")
    A = len(windows[0].news)
    if len(weights) != len(windows) or any(len(w) != A for w in weights):
        raise ValueError(f"{len(weights)} weight vectors for {len(windows)} texts of {A} attributes")
    retain = [""] if retain is None else [str(t) for t in retain]

    st.encode(retain)
    if st.E_old is None:
        st.E_old, st.E_att, st.row_seg = _stack_windows(st, windows, K)
        st.g_old = torch.zeros((K, K), device=dev, dtype=torch.float64)
        k.fid_accumulate(st.E_old[:st.row_seg[-1]], torch.zeros(K, device=dev, dtype=torch.float64), st.g_old)
    E_old, E_att, row_seg = st.E_old, st.E_att, st.row_seg
    m, mp = row_seg[-1], E_old.shape[0]
    mark("encode")

    key = (tuple(retain), float(lamb), float(erase_scale), float(preserve_scale))
    if key != st.system_key:
        scratch = torch.zeros(K, device=dev, dtype=torch.float64)
        g_ret = torch.zeros((K, K), device=dev, dtype=torch.float64)
        for s in range(0, len(retain), st.batch_size):
            k.fid_accumulate(torch.cat([st.emb[t] for t in retain[s:s + st.batch_size]]), scratch, g_ret)
        M = torch.empty((K, K), device=dev, dtype=torch.float64)
        info = torch.zeros(1, device=dev, dtype=torch.int32)
        k.spd_system(st.g_old, erase_scale, g_ret, preserve_scale, lamb, M)
        k.spd_factor(M, info)
        mark("gram_factor")
        Z = torch.zeros((mp, K), device=dev, dtype=torch.float32)
        k.spd_solve(M, E_old[:m], Z[:m])
        bad = int(info.item())
        if bad:
            raise RuntimeError(f"UCE debias: lam I + s_e G_old + s_r G_retain is not positive definite at column {bad - 1} "
                               f"(lam {lamb}, erase_scale {erase_scale}, preserve_scale {preserve_scale})")
        st.Z, st.system_key = Z, key
        st.factorisations += 1
        mark("solve")
    else:
        mark("gram_factor")
        mark("solve")
    Z = st.Z

    W = store.p("attn2_kv_all.weight")
    O = torch.empty((mp, ktot), device=dev, dtype=torch.float32)
    U = torch.empty((A, mp, ktot), device=dev, dtype=torch.float32)
    k.gemm(E_old, W, O, mp, ktot, K, K, K, ktot, dtype=k.F32)
    for j in range(A):
        k.gemm(E_att[j], W, U[j], mp, ktot, K, K, K, ktot, dtype=k.F32)
    mark("project")
    cols = kv_columns(unet)
    col_seg = [c for _n, c, _r in cols] + [cols[-1][1] + cols[-1][2]]
    if col_seg[0] != 0 or col_seg[-1] != ktot or any(a + r != b for (_n, a, r), b in zip(cols, col_seg[1:])):
        raise RuntimeError("attn2_kv_all: the projections do not tile the matrix' rows")
    w_dev = torch.stack([torch.as_tensor(w, dtype=torch.float32) for w in weights]).contiguous().to(dev)
    D = torch.empty((mp, ktot), device=dev, dtype=torch.float32)
    k.uce_debias_delta(O, U, D, w_dev, row_seg, col_seg)
    mark("delta")
    # W_all [ktot, K] += s_e D^T Z: the weight-gradient form, reduction over the (zero-padded) rows
    k.gemm(D, Z, W, ktot, K, mp, ktot, K, K, a_mode=k.A_COLK, b_mode=k.B_COLK, dtype=k.F32, out_f32=True, accumulate=True,
           alpha=float(erase_scale))
    store.refresh()
    mark("update")
    return unet


@torch.no_grad()
def debias_model(pipe, clip, clip_tokenizer, old_texts, new_texts, retain_texts, rng, num_images=10, resolution=768,
                 settings=None, max_iterations=None, num_seeds=None, steps=None, stages=None, timing=None):
    """The reference's outer loop on pipe.unet: measure, stop when every concept is within max_bias_diff of uniform, else
    derive the weights and the retain list (schedule) and edit - at most max_iterations times.  rng: the np.random.RandomState
    the num_seeds sampling seeds of every measurement come from.  retain_texts None: [''].  Returns (weights, init_ratios,
    ratios, iterations): the weights of the last edit (zeros without one), the first and the last measurement, and the number
    of measurements made.  store.refresh() runs inside every edit, so the captured sampler of the next measurement reads the
    edited weights."""
    s = settings or load_settings()
    gap, step_w = float(s["max_bias_diff"]), float(s["weight_step"])
    max_iterations = int(s["max_iterations"] if max_iterations is None else max_iterations)
    num_seeds = int(s["num_seeds"] if num_seeds is None else num_seeds)
    steps = int(s["num_inference_steps"] if steps is None else steps)
    print(old_texts, new_texts)
    state, windows = prepare(pipe.text_encoder, pipe.tokenizer, old_texts, new_texts, pipe.device)
    retain = [""] if retain_texts is None else list(retain_texts)
    weights = [torch.zeros(len(c)) for c in new_texts]
    ratios = prev = prev_change = bypass = init_ratios = None
    iterations = 0
    for i in range(max_iterations):
        seeds = rng.randint(int(s["seed_range"]), size=num_seeds)
        ratios = get_ratios(pipe, clip, clip_tokenizer, old_texts, new_texts, bypass, prev, seeds, num_images, steps, resolution,
                            guidance_scale=float(s["guidance_scale"]), timing=timing)
        iterations = i + 1
        if i == 0:
            init_ratios = ratios
        print(ratios)
        step = schedule(ratios, prev, prev_change, retain, old_texts, gap, step_w)
        if step.done:
            print(f"All concepts are debiased at Iteration:{i}")
            break
        retain, weights = step.retain_texts, step.weights
        debias_edit(pipe.unet, state, windows, weights, retain, lamb=float(s["lamb"]), erase_scale=float(s["erase_scale"]),
                    preserve_scale=float(s["preserve_scale"]), stages=stages)
        prev, prev_change, bypass = ratios, step.max_change, step.bypass
    print(f'Current model status: Edited "{old_texts}" into "{new_texts}" and Retained {len(retain)} texts')
    return weights, init_ratios, ratios, iterations


# ---- CLIP_classify.py (GPU)
@torch.no_grad()
def classify_folder(clip, tokenizer, im_path, attributes, prompts_path, save_path=None, from_case=0, till_case=1000000000,
                    batch_size=64):
    """eval-scripts/CLIP_classify.py over a folder: <save_path>/<folder>_gender_classify.csv, the prompts frame plus one
    `<attribute>_bias` column per attribute holding the mean mask of the case's images, and (path, header, rows) as written.
    Files: names containing `.png`, in sorted_nicely order, the case number in front of the first `_`, kept when inside
    [from_case, till_case]; a file that cannot be decoded counts as a row of zeros.  The frame is joined as
    object_erasure.merge_on_case_number does it (a case without images drops out; the reference writes through df.loc[case],
    the row *label*).  Means are hits / files in fp64."""
    from .. import _pdmk as k
    from .clip_utils import pack_images, prep_images, tokenize
    from .data import open_rgb
    from .object_erasure import merge_on_case_number
    from .perceptual import read_frame
    folder = os.path.basename(os.path.abspath(im_path))
    if save_path is None:
        save_path = im_path.replace(folder, "")
    print(folder, attributes, save_path)
    header, rows = read_frame(prompts_path)
    names = sorted_nicely([n for n in os.listdir(im_path) if ".png" in n])
    names = [n for n in names if from_case <= png_case_number(n) <= till_case]
    cases = list(dict.fromkeys(png_case_number(n) for n in names))
    files = {c: 0 for c in cases}
    A, R, dev = len(attributes), clip.image_size, clip.device
    hits = torch.zeros((max(len(cases), 1), A), device=dev, dtype=torch.int32)
    classes = clip.encode_text(tokenize(tokenizer, list(attributes), context_length=clip.context_length))
    good = []
    for n in names:
        files[png_case_number(n)] += 1
        a = open_rgb(os.path.join(im_path, n))
        if a is not None:
            good.append((cases.index(png_case_number(n)), a))
    bs = max(int(batch_size), 1)
    for s in range(0, len(good), bs):
        part = good[s:s + bs]
        packed, desc = pack_images([a for _c, a in part], R)
        img = clip.encode_image(prep_images(packed, desc, R, dev))
        group = torch.tensor([c for c, _a in part], dtype=torch.int32).to(dev)
        k.zeroshot_head(img, classes, logit_scale(clip), group=group, hits=hits)
    counts = hits.cpu().numpy().astype(np.float64)
    result_rows = [[c] + [float(counts[i, a] / files[c]) for a in range(A)] for i, c in enumerate(cases)]
    out_header, out_rows = merge_on_case_number(header, rows, ["case_number"] + bias_columns(attributes), result_rows)
    path = write_csv(os.path.join(save_path, f"{folder}_gender_classify.csv"), out_header, out_rows)
    return path, out_header, out_rows
