"""Unified Concept Editing on the pruned student (the reference's baselines/unified-concept-editing/train-scripts/
train_erase.py): a closed-form edit of every cross-attention `attn2.to_k` / `attn2.to_v` weight that maps the text embeddings of
the concepts to erase onto the projections of the guiding texts while keeping the projections of the retained texts.  No
training.

The reference computes, per projection W [O, K],  W' = mat1 inverse(mat2)  with
    mat1 = lam W + s_e sum V^T E_old + s_r sum (E_r W^T)^T E_r,     mat2 = lam I + s_e sum E_old^T E_old + s_r sum E_r^T E_r.
mat1 = W mat2 + s_e sum (V - O)^T E_old with O = E_old W^T, so the retain terms cancel and
    W' = W + s_e D^T Z,     D = V - O  [m, O],     Z = E_old mat2^-1  [m, K]
over the m erase rows of all pairs.  mat2 does not depend on the projection: it is formed once from two Gram matrices
(pdmk_fid_accumulate, fp64), factored once (pdmk_spd_factor_f64) and solved for the m rows (pdmk_spd_solve_f64), in fp64;
O, N for all projections are two fp32 GEMMs against the one master matrix `attn2_kv_all` that holds every to_k / to_v as a row
block, D comes from pdmk_uce_delta and the update is one more GEMM on that matrix.  Every distinct text is encoded once.

Host side (no GPU needed): the text-list builders, the checkpoint name, the slice arithmetic.  GPU side: `edit_model`.

Built elsewhere: train_debias.py (a loop of generation, CLIP classification and this edit with other targets) and
CLIP_classify.py in pdm/utils/uce_debias.py; generate-images.py, lpips_eval.py and styleloss.py in pdm/utils/perceptual.py;
imageclassify.py in pdm/utils/object_erasure.py.  Not built: the NudeNet-based eval-scripts, `layers_to_edit` (the reference's
__main__ never sets it), SD-1.4, and the fixed concept lists `allartist`, `i2g`, `10artists`, `imagenette`.
"""
import random

import torch

from .load_models import golden_path

LAMB = 0.5
FIXED_LISTS = ("allartist", "i2g", "10artists", "imagenette")
TECHNIQUES = ("replace", "tensor")
ROW_PAD = 64                      # erase rows are zero-padded to a multiple of this for the update GEMM's reduction


# ---- flags, texts and names (train_erase.py:355-451, :479-481)
def default_artists_file():
    return golden_path("uce", "artists1734.txt")


def read_artists(path=None):
    """The unique artists of the reference's artists1734_prompts.csv in order of first appearance, one per line."""
    with open(path or default_artists_file(), encoding="utf-8") as f:
        names = [line.rstrip("\n") for line in f]
    names = [n for n in names if n]
    if not names:
        raise ValueError(f"{path}: no artists")
    return names


def additional_prompts(concept_type):
    """The five `{concept}` templates of --add_prompts for `art` / `object`, none for any other type."""
    if concept_type == "art":
        return [f"{w} by {{concept}}" for w in ("painting", "art", "artwork", "picture")] + ["style of {concept}"]
    if concept_type == "object":
        return [f"{w} of {{concept}}" for w in ("image", "photo", "portrait", "picture", "painting")]
    return []


def split_list(text):
    return [c.strip() for c in text.split(",")]


def build_texts(concepts, concept_type, guided_concepts=None, preserve_concepts=None, preserve_number=None, add_prompts=False,
                technique="replace", base="2.1", seed=0, artists=None):
    """(concepts, old_texts, new_texts, retain_texts, name) by the reference's rules.  `concepts`, `guided_concepts`,
    `preserve_concepts`: the comma-separated flag strings (or None).  random.sample runs on random.Random(seed), `<N>artists`
    first and --preserve_number second (the reference samples unseeded).  A --preserve_concepts string is split at commas (the
    reference adds the string to a list and raises)."""
    if technique not in TECHNIQUES:
        raise ValueError(f"--technique {technique!r}: expected one of {', '.join(TECHNIQUES)}")
    if str(base) != "2.1":
        raise NotImplementedError(f"--base {base}: only 2.1 (the pruned SD-2.1 student) is built here")
    rng = random.Random(seed)
    concepts = split_list(concepts)
    name = "_".join(c.lower() for c in concepts)
    if concepts[0] in FIXED_LISTS:
        raise NotImplementedError(f"--concepts {concepts[0]}: the reference's fixed concept lists are not built here; "
                                  f"name the concepts")
    if "artists" in concepts[0]:
        number = int(concepts[0].replace("artists", ""))
        concepts = rng.sample(artists if artists is not None else read_artists(), number)

    templates = additional_prompts(concept_type) if add_prompts else []
    length = 1 + len(templates)
    old_texts = []
    for concept in concepts:
        old_texts.append(f"{concept}")
        old_texts += [t.format(concept=concept) for t in templates]

    if guided_concepts is None:
        new_texts = [" " for _ in old_texts]
        name += "-towards_uncond"
    else:
        guided = split_list(guided_concepts)
        if len(guided) == 1:
            new_texts = [guided[0] for _ in old_texts]
            name += f"-towards_{guided[0]}"
        else:
            new_texts = [g for g in guided for _ in range(length)]
            name += "-towards"
            for t in new_texts:
                if t not in name:
                    name += f"-{t}"
    if len(new_texts) != len(old_texts):
        raise ValueError(f"{len(new_texts)} guiding texts for {len(old_texts)} texts to erase: give one guided concept, or one "
                         f"per concept")

    if preserve_concepts is None:
        preserve = []
        if concept_type == "art":
            lower = [t.lower() for t in old_texts]
            preserve = [a for a in (artists if artists is not None else read_artists()) if a.lower() not in lower]
            if preserve_number is not None:
                name += f"-preserving_{preserve_number}artists"
                preserve = rng.sample(preserve, preserve_number)
    else:
        preserve = split_list(preserve_concepts) if isinstance(preserve_concepts, str) else list(preserve_concepts)
    retain_texts = [""] + preserve
    name += "-preserve_true" if len(retain_texts) > 1 else "-preserve_false"
    name += f"-sd_{str(base).replace('.', '_')}-method_{technique}"
    return concepts, old_texts, new_texts, retain_texts, name.lower()


def default_preserve_scale(preserve_scale, retain_texts):
    return max(0.1, 1 / len(retain_texts)) if preserve_scale is None else preserve_scale


def add_arguments(parser):
    """The reference's flags and this build's additions (--model_id, --output_dir, --seed, --tiny).  Prefix matching stays on:
    the reference's run.sh spells --guided_concepts as --guided_concept."""
    parser.add_argument("--concepts", help="prompt corresponding to concept to erase", type=str, required=True)
    parser.add_argument("--guided_concepts", help="Concepts to guide the erased concepts towards", type=str, default=None)
    parser.add_argument("--preserve_concepts", help="Concepts to preserve", type=str, default=None)
    parser.add_argument("--technique", help="technique to erase (either replace or tensor)", type=str, default="replace")
    parser.add_argument("--device", help="cuda devices to train on", type=str, default="0")
    parser.add_argument("--base", help="base version for stable diffusion", type=str, default="2.1")
    parser.add_argument("--preserve_scale", help="scale to preserve concepts", type=float, default=None)
    parser.add_argument("--preserve_number", help="number of preserve concepts", type=int, default=None)
    parser.add_argument("--erase_scale", help="scale to erase concepts", type=float, default=1)
    parser.add_argument("--concept_type", help="type of concept being erased", type=str, required=True)
    parser.add_argument("--add_prompts", help="option to add additional prompts (any non-empty string is true)", type=bool,
                        default=False)
    parser.add_argument("--base_config_path", help="Path to base config file", type=str)
    parser.add_argument("--ckpt_path", help="Path to checkpoint file", type=str)
    parser.add_argument("--model_id", type=str, default=None, help="SD-2.1 snapshot directory (tokenizer, text encoder)")
    parser.add_argument("--output_dir", type=str, default=".", help="models/ and info/ are written below it")
    parser.add_argument("--seed", type=int, default=0, help="seed of random.sample (<N>artists, --preserve_number)")
    parser.add_argument("--tiny", action="store_true", help="tiny U-Net topology (tests)")
    return parser


# ---- slices
def pair_slices(n_old, n_new, length):
    """((start, stop) of the old text's rows, (start, stop) of the new text's) from the attention-mask sums n (BOS + words + EOS)
    of a pair padded to `length` tokens: from the last word token on, cut so that both have length - max(n_old, n_new) + 2 rows."""
    f_old, f_new = n_old - 2, n_new - 2
    far = max(f_old, f_new)
    return (f_old, length - (far - f_old)), (f_new, length - (far - f_new))


def kv_columns(unet):
    """[(state-dict name, first row, rows)] of every attn2.to_k / to_v inside the master matrix attn2_kv_all, in row order."""
    e = unet.store.by_key["attn2_kv_all.weight"]
    return sorted(((name, d0, rows) for name, rows, d0, _s0 in e.srcs), key=lambda t: t[1])


# ---- the edit (GPU)
def _encode(text_encoder, ids, device):
    return text_encoder(ids.to(device))[0].to(torch.float32)


@torch.no_grad()
def edit_model(unet, text_encoder, tokenizer, old_texts, new_texts, retain_texts, lamb=LAMB, erase_scale=1.0,
               preserve_scale=0.1, technique="replace", batch_size=64, stages=None):
    """Edits the fp32 master weights of every attn2.to_k / to_v of `unet` in place (module docstring) and refreshes the compute
    copies.  retain_texts None: [''] (the reference's retain=False).  Only the factorisation's info flag is read back; a pivot
    that is not positive raises before any weight is touched.  stages: a callable(name) called between the stages (timing)."""
    from .. import _pdmk as k
    if technique not in TECHNIQUES:
        raise ValueError(f"technique {technique!r}: expected one of {', '.join(TECHNIQUES)}")
    mark = stages or (lambda name: None)
    dev = unet.device
    store = unet.store
    if not store.has("attn2_kv_all.weight"):
        raise ValueError("the model has no cross-attention left to edit")
    e = store.by_key["attn2_kv_all.weight"]
    ktot, Kp = e.shape
    K = e.logical[1]
    if K != Kp or K % 16:
        raise NotImplementedError(f"cross_attention_dim {K}: the fp32 GEMM loaders need a multiple of 16")
    old_texts = list(old_texts)
    new_texts = [" " if t == "" else t for t in new_texts]
    retain_texts = [""] if retain_texts is None else list(retain_texts)
    if len(old_texts) != len(new_texts) or not old_texts:
        raise ValueError(f"{len(old_texts)} texts to erase, {len(new_texts)} guiding texts")

    # every distinct text once: the erase texts are kept, the retain texts stream through the Gram
    erase = list(dict.fromkeys(old_texts + new_texts))
    tok = tokenizer(erase, padding="max_length", max_length=tokenizer.model_max_length, truncation=True, return_tensors="pt")
    T = tok.input_ids.shape[1]
    count = dict(zip(erase, tok.attention_mask.sum(1).tolist()))
    emb = {}
    bs = max(int(batch_size), 1)
    for s in range(0, len(erase), bs):
        y = _encode(text_encoder, tok.input_ids[s:s + bs], dev)
        emb.update(zip(erase[s:s + bs], y))
    mark("encode_erase")

    row_seg, olds, news = [0], [], []
    for o, n in zip(old_texts, new_texts):
        (a0, a1), (b0, b1) = pair_slices(count[o], count[n], T)
        olds.append(emb[o][a0:a1])
        news.append(emb[n][b0:b1])
        row_seg.append(row_seg[-1] + a1 - a0)
    m = row_seg[-1]
    mp = (m + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    E_old = torch.zeros((mp, K), device=dev, dtype=torch.float32)
    E_new = torch.zeros((mp, K), device=dev, dtype=torch.float32)
    E_old[:m] = torch.cat(olds)
    E_new[:m] = torch.cat(news)

    scratch = torch.zeros(K, device=dev, dtype=torch.float64)
    g_old = torch.zeros((K, K), device=dev, dtype=torch.float64)
    g_ret = torch.zeros((K, K), device=dev, dtype=torch.float64)
    k.fid_accumulate(E_old[:m], scratch, g_old)
    uniq = list(dict.fromkeys(retain_texts))
    times = {}
    for t in retain_texts:
        times[t] = times.get(t, 0) + 1
    fresh = [t for t in uniq if t not in emb]
    have = [emb[t] for t in uniq if t in emb for _ in range(times[t])]
    if have:
        k.fid_accumulate(torch.cat(have), scratch, g_ret)
    for s in range(0, len(fresh), bs):
        part = fresh[s:s + bs]
        ids = tokenizer(part, padding="max_length", max_length=tokenizer.model_max_length, truncation=True,
                        return_tensors="pt").input_ids
        y = _encode(text_encoder, ids, dev)
        rep = [i for i, t in enumerate(part) for _ in range(times[t])]
        if len(rep) != len(part):
            y = y[torch.tensor(rep, device=dev)]
        k.fid_accumulate(y.reshape(-1, K), scratch, g_ret)
    mark("encode_retain_gram")

    A = torch.empty((K, K), device=dev, dtype=torch.float64)
    info = torch.zeros(1, device=dev, dtype=torch.int32)
    k.spd_system(g_old, erase_scale, g_ret, preserve_scale, lamb, A)
    k.spd_factor(A, info)
    mark("system_factor")
    Z = torch.zeros((mp, K), device=dev, dtype=torch.float32)
    k.spd_solve(A, E_old[:m], Z[:m])
    bad = int(info.item())
    if bad:
        raise RuntimeError(f"UCE: lam I + s_e G_old + s_r G_retain is not positive definite at column {bad - 1} "
                           f"(lam {lamb}, erase_scale {erase_scale}, preserve_scale {preserve_scale})")
    mark("solve")

    W = store.p("attn2_kv_all.weight")
    O = torch.empty((mp, ktot), device=dev, dtype=torch.float32)
    N = torch.empty((mp, ktot), device=dev, dtype=torch.float32)
    k.gemm(E_old, W, O, mp, ktot, K, K, K, ktot, dtype=k.F32)
    k.gemm(E_new, W, N, mp, ktot, K, K, K, ktot, dtype=k.F32)
    mark("project")
    cols = kv_columns(unet)
    col_seg = [c for _n, c, _r in cols] + [cols[-1][1] + cols[-1][2]]
    if col_seg[0] != 0 or col_seg[-1] != ktot or any(a + r != b for (_n, a, r), b in zip(cols, col_seg[1:])):
        raise RuntimeError("attn2_kv_all: the projections do not tile the matrix' rows")
    D = torch.empty((mp, ktot), device=dev, dtype=torch.float32)
    k.uce_delta(O, N, D, row_seg, col_seg, TECHNIQUES.index(technique))
    mark("delta")
    # W_all [ktot, K] += s_e D^T Z: the weight-gradient form, reduction over the (zero-padded) erase rows
    k.gemm(D, Z, W, ktot, K, mp, ktot, K, K, a_mode=k.A_COLK, b_mode=k.B_COLK, dtype=k.F32, out_f32=True, accumulate=True,
           alpha=float(erase_scale))
    store.refresh()
    mark("update")
    print(f'Current model status: Edited "{old_texts}" into "{new_texts}" and Retained {len(retain_texts)} texts')
    return unet
