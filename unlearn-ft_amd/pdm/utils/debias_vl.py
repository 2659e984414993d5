"""Debias-VL (Chuang et al. 2023) as the reference's baselines/unified-concept-editing/eval-scripts/debiasing_vl.py uses it: a
calibration matrix applied to the conditional prompt embeddings.  No weight changes.

    z        L2-normalised EOS-token embeddings (the EOS row is the argmax of the ids) of `A photo of a male {c}.` /
             `A photo of a female {c}.`, c lower-cased, for every concept c
    M        (1 / |S|) sum_s (z_i - z_j)(z_i - z_j)^T over the pairs s = (male, female)
    P        inv(500 M + I);  text_embeddings @ P^T on the conditional embeddings only

Here: pdmk_gather_rows and pdmk_clip_score_head form z, pdmk_pair_gram_f64 forms 500 M + I in fp64, pdmk_spd_factor_f64 factors
it once per run and pdmk_spd_solve_f64 gives X (L L^T)^-1 = X P^T (P is symmetric) for the 77 rows of one prompt; no inverse is
formed.  The constant, the two templates and the default concept list are data in configs/baselines/debias_vl.yaml.
"""
import os

import torch


def settings_path():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "configs", "baselines",
                        "debias_vl.yaml")


def load_settings(path=None):
    """{"lam": float, "templates": [male, female], "concepts": [...]} of the settings YAML."""
    import yaml
    with open(path or settings_path(), encoding="utf-8") as f:
        settings = yaml.safe_load(f)
    if len(settings["templates"]) != 2 or not settings["concepts"]:
        raise ValueError(f"{path or settings_path()}: expected two templates and a non-empty concept list")
    return settings


def split_concepts(text, settings=None):
    """`--debias_concepts`: comma separated, stripped; empty means the settings' default list (debiasing_vl.py:178-182)."""
    concepts = [c.strip() for c in str(text).split(",")]
    if concepts == [""]:
        return list((settings or load_settings())["concepts"])
    return concepts


def build_prompts(concepts, settings=None):
    """[male(c0), female(c0), male(c1), ...] with c lower-cased (debiasing_vl.py:63-67): pair p is rows 2p, 2p + 1."""
    male, female = (settings or load_settings())["templates"]
    prompts = []
    for c in concepts:
        c = str(c).lower()
        prompts += [male.format(c), female.format(c)]
    return prompts


class Factor:
    """The Cholesky factor L of 500 M + I (fp64 [d, d], lower triangle) and the normalised embeddings z it came from."""

    def __init__(self, L, z, info):
        self.L, self.z, self.info = L, z, info

    @property
    def d(self):
        return self.L.shape[0]


@torch.no_grad()
def pooled_normalised(text_encoder, ids, device):
    """L2-normalised EOS rows (fp32 [n, ctx]) of the text encoder's last hidden state for token ids [n, T]."""
    from .. import _pdmk as k
    ids = ids.to(device, torch.int64).contiguous()
    n, T = ids.shape
    y = text_encoder(ids)[0]
    ctx = y.shape[-1]
    y = y.reshape(n * T, ctx).contiguous()
    eos = torch.empty((n, ctx), device=device, dtype=y.dtype)
    k.gather_rows(y, ids, T, eos, n, ctx)
    eos = eos.to(torch.float32)
    z = torch.empty((n, ctx), device=device, dtype=torch.float32)
    k.clip_score_head(eos, None, z, None, None, n, ctx)
    return z


def factor_from_pairs(z, lam):
    """z fp32 [2 * pairs, d] on the device -> Factor of lam M + I; raises when a pivot is not positive and finite."""
    from .. import _pdmk as k
    pairs, d = z.shape[0] // 2, z.shape[1]
    A = torch.empty((d, d), device=z.device, dtype=torch.float64)
    info = torch.zeros(1, device=z.device, dtype=torch.int32)
    k.pair_gram(z, float(lam) / pairs, 1.0, A)
    k.spd_factor(A, info)
    if int(info.item()) != 0:
        raise ArithmeticError(f"debias-VL: the calibration system is not positive definite (column {int(info.item()) - 1})")
    return Factor(A, z, info)


@torch.no_grad()
def calibration(frozen, concepts, settings=None, batch_size=64):
    """The factor of one run: `frozen` supplies text_encoder, tokenizer and device (load_models.FrozenModels)."""
    settings = settings or load_settings()
    prompts = build_prompts(concepts, settings)
    tok, enc, dev = frozen.tokenizer, frozen.text_encoder, frozen.device
    parts = []
    for s in range(0, len(prompts), batch_size):
        ids = tok(prompts[s:s + batch_size], padding="max_length", max_length=tok.model_max_length, truncation=True,
                  return_tensors="pt").input_ids
        parts.append(pooled_normalised(enc, ids, dev))
    return factor_from_pairs(torch.cat(parts).contiguous(), settings["lam"])


@torch.no_grad()
def apply(factor, embeds):
    """embeds [..., d] (any float dtype, on the factor's device) -> embeds @ P^T in the same shape and dtype: the rows solved
    in fp64 from their exact fp32 values, rounded once to fp32, then cast."""
    from .. import _pdmk as k
    if embeds.shape[-1] != factor.d:
        raise ValueError(f"debias-VL: embeddings are {embeds.shape[-1]} wide, the calibration {factor.d}")
    B = embeds.to(factor.L.device, torch.float32).reshape(-1, factor.d).contiguous()
    X = torch.empty_like(B)
    k.spd_solve(factor.L, B, X)
    return X.reshape(embeds.shape).to(embeds.dtype)
