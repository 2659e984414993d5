#!/usr/bin/env python3
"""UCE edit, stage by stage, at SD-2.1 shapes on one MI355X: dense U-Net topology (attn2_kv_all [ktot, 1024]) and the SD-2.1 text
encoder, both fp32 with random weights; a stand-in tokenizer (seeded token ids, lengths from the word count) since no
vocabulary file is needed to time anything.
  (a) one concept, no retain list           (b) one concept with the 1734-artist retain list
  stages of edit_model (second run of each; the first one tunes GEMM plans and captures the encoder's graphs), the Gram of the
  same number of rows on its own, and pdmk_spd_factor_f64 + pdmk_spd_solve_f64 beside torch.linalg.cholesky + cholesky_solve
  in fp64 on the same tensors.
One line per measurement; nothing is asserted."""
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unlearn-ft_amd"))
import torch
from pdm import _pdmk as k
from pdm.models.clip.text_encoder import CLIPTextModel
from pdm.models.unet.spec import UNetConfig
from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
from pdm.utils import uce as U

dev = torch.device("cuda:0")
T, K = 77, 1024


class Tokens:
    """tokenizer(texts, ...) -> input_ids [B, 77], attention_mask: BOS, two seeded ids per word (at most 75), EOS, padding."""
    model_max_length = T

    def __call__(self, texts, **unused):
        ids = torch.zeros((len(texts), T), dtype=torch.int64)
        mask = torch.zeros((len(texts), T), dtype=torch.int64)
        for i, t in enumerate(texts):
            words = [w for w in t.split(" ") if w]
            body = [zlib.crc32(f"{w}/{j}".encode()) % 49000 + 1 for w in words for j in (0, 1)][:T - 2]
            row = [49406] + body + [49407]
            ids[i, :len(row)] = torch.tensor(row)
            mask[i, :len(row)] = 1
        return type("Enc", (), {"input_ids": ids, "attention_mask": mask})()


def events(fn, rep=3):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rep): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / rep


cfg = UNetConfig.sd21()
enc = CLIPTextModel(None, dev, torch.float32, seed=1)
tok = Tokens()
artists = U.read_artists()

for label, retain in (("(a) one concept, retain ['']", [""]), ("(b) one concept, retain [''] + 1733 artists",
                                                              [""] + [a for a in artists if a != "Vincent Van Gogh"])):
    unet = UNet2DConditionModelPruned(cfg, None, dev, torch.float32, train=False, seed=0)
    ktot = unet.store.by_key["attn2_kv_all.weight"].shape[0]
    for run in range(2):
        marks = []

        def mark(name):
            torch.cuda.synchronize()
            marks.append((name, time.perf_counter()))

        mark("start")
        U.edit_model(unet, enc, tok, ["Vincent Van Gogh"], ["art"], retain, erase_scale=1.0,
                     preserve_scale=U.default_preserve_scale(None, retain), stages=mark)
    rows = T * len(retain)
    print(f"== {label}: K = {K}, ktot = {ktot} rows of attn2_kv_all in {len(U.kv_columns(unet))} projections, {rows} retain rows")
    for (_, t0), (name, t1) in zip(marks, marks[1:]):
        print(f"   {name:20s} {(t1 - t0) * 1e3:9.3f} ms", flush=True)
    print(f"   {'total':20s} {(marks[-1][1] - marks[0][1]) * 1e3:9.3f} ms")
    # the Gram of as many rows on its own, in the edit's batches of 64 texts
    x = torch.randn(64 * T, K, device=dev)
    g, s = torch.zeros((K, K), device=dev, dtype=torch.float64), torch.zeros(K, device=dev, dtype=torch.float64)
    nb = (len(retain) + 63) // 64
    ms = events(lambda: k.fid_accumulate(x, s, g))
    print(f"   pdmk_fid_accumulate, {64 * T} x {K} rows: {ms:7.3f} ms per batch, {nb} batches = {ms * nb:8.3f} ms of the stage "
          f"encode_retain_gram")
    del unet

print(f"== factor + solve, n = {K}, fp64, against torch on the same tensors")
for m in (75, 450):
    g = torch.Generator(device=dev).manual_seed(m)
    E = torch.randn(m, K, device=dev, generator=g)
    R = torch.randn(4096, K, device=dev, generator=g)
    A0 = 0.5 * torch.eye(K, device=dev, dtype=torch.float64) + E.double().T @ E.double() + 0.1 * R.double().T @ R.double()
    A, info = A0.clone(), torch.zeros(1, device=dev, dtype=torch.int32)
    X, X64 = torch.empty((m, K), device=dev), torch.empty((m, K), device=dev, dtype=torch.float64)

    def factor():
        A.copy_(A0)
        k.spd_factor(A, info)

    t_copy = events(lambda: A.copy_(A0))
    t_factor = events(factor) - t_copy
    t_solve = events(lambda: k.spd_solve(A, E, X, X64))
    assert int(info.item()) == 0
    try:
        t_chol = events(lambda: torch.linalg.cholesky(A0))
        Lt = torch.linalg.cholesky(A0)
        t_csol = events(lambda: torch.cholesky_solve(E.double().T, Lt))
        Xt = torch.cholesky_solve(E.double().T, Lt).T
        where = "torch on the device"
    except RuntimeError as err:
        print(f"   torch has no device solver here ({str(err).splitlines()[0][:80]}): torch on the CPU")
        Ac, Ec = A0.cpu(), E.double().cpu()
        t0 = time.perf_counter(); Lt = torch.linalg.cholesky(Ac); t_chol = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter(); Xt = torch.cholesky_solve(Ec.T, Lt).T; t_csol = (time.perf_counter() - t0) * 1e3
        Xt = Xt.to(dev)
        where = "torch on the CPU"
    diff = float((X64 - Xt).abs().max() / Xt.abs().max())
    print(f"   m = {m:4d}: pdmk factor {t_factor:7.3f} ms + solve {t_solve:7.3f} ms = {t_factor + t_solve:7.3f} ms;   {where}: "
          f"cholesky {t_chol:7.3f} ms + cholesky_solve {t_csol:7.3f} ms = {t_chol + t_csol:7.3f} ms;   max |X - X_torch| / max |X| "
          f"{diff:.2e}", flush=True)
