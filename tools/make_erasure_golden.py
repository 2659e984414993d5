"""Writes tests/golden/artist_erasure_hf.npz (+ .report.txt): what the reference's artist_erasure.py:136-163 computes with
transformers.CLIPModel in fp32 on the CPU, for the tiny seeded weights of tests/clip_score_fixtures.py - the independent
reference of scripts/metrics/artist_erasure.py's scoring stage.  Inputs are not stored: the test regenerates them from the
same seeds (the first 8 E2E_CAPTIONS; originals image_array(64, 64, 2015 + i), removals image_array(64, 64, 2023 + i)).

  sim_orig, sim_removed   F.cosine_similarity(text features, image features) per pair, fp32 [8]
  score                   1 where sim_removed < sim_orig, int64 [8]
  avg_similarity, std_similarity, avg_score, std_score   np.mean / np.std as the reference takes them

The script refuses inputs on which the comparison is fragile: the smallest |sim_removed - sim_orig| must be >= 4e-3 (four
times the test's per-pair tolerance of 1e-3) and the flags must not all be equal.

Run: python tools/make_erasure_golden.py   (deterministic: regenerates the committed file bit for bit)
"""
import io
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import clip_score_fixtures as fx
from make_clip_score_golden import hf_model, image_features, text_features

N = 8
ORIG_SEED, REMOVED_SEED, SIDE = 2015, 2023, 64
MIN_MARGIN = 4e-3


def inputs():
    captions = fx.E2E_CAPTIONS[:N]
    originals = [fx.image_array(SIDE, SIDE, ORIG_SEED + i) for i in range(N)]
    removals = [fx.image_array(SIDE, SIDE, REMOVED_SEED + i) for i in range(N)]
    return captions, originals, removals


@torch.no_grad()
def reference(m, tmp):
    from transformers import CLIPTokenizer
    captions, originals, removals = inputs()
    d = fx.write_tokenizer(os.path.join(tmp, "tok"))
    tok = CLIPTokenizer.from_pretrained(os.path.join(d, "tokenizer"), local_files_only=True)
    sim_orig, sim_removed, scores = [], [], []
    for cap, o, r in zip(captions, originals, removals):            # one pair at a time, as the reference
        ids = np.asarray([tok(cap)["input_ids"]], np.int64)
        tf = text_features(m, ids)
        so = torch.nn.functional.cosine_similarity(tf, image_features(m, [o]))
        sr = torch.nn.functional.cosine_similarity(tf, image_features(m, [r]))
        sim_orig.append(so.item())
        sim_removed.append(sr.item())
        scores.append(1 if sr < so else 0)
    return sim_orig, sim_removed, scores


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)              # fixed reduction order: the file regenerates bit for bit
    with tempfile.TemporaryDirectory() as tmp:
        sim_orig, sim_removed, scores = reference(hf_model("tiny"), tmp)
    margin = float(np.abs(np.asarray(sim_removed) - np.asarray(sim_orig)).min())
    assert margin >= MIN_MARGIN, f"smallest |sim_removed - sim_orig| {margin:.2e} < {MIN_MARGIN:.0e}: choose other seeds"
    assert 0 < sum(scores) < N, f"all flags equal ({scores}): choose other seeds"
    out = {"sim_orig": np.asarray(sim_orig, np.float32), "sim_removed": np.asarray(sim_removed, np.float32),
           "score": np.asarray(scores, np.int64),
           "avg_similarity": np.float64(np.mean(sim_removed)), "std_similarity": np.float64(np.std(sim_removed)),
           "avg_score": np.float64(np.mean(scores)), "std_score": np.float64(np.std(scores))}
    import transformers
    report = [f"transformers {transformers.__version__}, torch {torch.__version__}, fp32 CPU",
              f"tiny: text {fx.CONFIGS['tiny'][0]} vision {fx.CONFIGS['tiny'][1]} projection {fx.CONFIGS['tiny'][2]}",
              f"  {N} pairs of {SIDE} x {SIDE} images, seeds {ORIG_SEED}+i / {REMOVED_SEED}+i",
              "  sim_orig    " + " ".join(f"{v:+.5f}" for v in sim_orig),
              "  sim_removed " + " ".join(f"{v:+.5f}" for v in sim_removed),
              f"  score {scores} ({sum(scores)} of {N} set), smallest margin {margin:.2e}",
              f"  avg_similarity {out['avg_similarity']:.6f} std_similarity {out['std_similarity']:.6f} "
              f"avg_score {out['avg_score']:.4f} std_score {out['std_score']:.6f}"]
    gold = os.path.join(ROOT, "tests", "golden", "artist_erasure_hf.npz")
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    with open(gold, "wb") as f:
        f.write(buf.getvalue())
    with open(gold.replace(".npz", ".report.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
    print(f"wrote {gold} ({os.path.getsize(gold)} bytes)")


if __name__ == "__main__":
    main()
