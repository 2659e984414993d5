"""Writes tests/golden/clip_score_hf.npz (+ .report.txt): outputs of transformers.CLIPModel in fp32 on the CPU for the seeded
weights of tests/clip_score_fixtures.py - the independent reference of the HIP CLIP model and score.  Inputs are not stored:
the tests regenerate them from the same seeds.

  {tiny,b32}_img   projected image features of model_images() after the CPU CLIP transform (PIL bicubic + normalisation)
  {tiny,b32}_txt   projected text features of text_ids()
  e2e_txt          normalised text features of the script test's captions (tiny model, fixture tokenizer), sorted by stem
  e2e_score        logit_scale.exp() * mean cos(text, image) over the script test's 12 images

Run: python tools/make_clip_score_golden.py   (deterministic: regenerates the committed file bit for bit)
"""
import io
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import clip_score_fixtures as fx


def hf_model(tag):
    from transformers import CLIPConfig, CLIPModel
    text, vision, proj = fx.CONFIGS[tag]
    V = text["vocab_size"]
    cfg = CLIPConfig(text_config=dict(text, bos_token_id=V - 2, eos_token_id=V - 1, pad_token_id=V - 1),
                     vision_config=dict(vision), projection_dim=proj)
    m = CLIPModel(cfg).eval().float()
    sd = fx.state_dict(tag)
    own = m.state_dict()
    missing = [n for n in own if n not in sd and not n.endswith("position_ids")]
    assert not missing, missing
    m.load_state_dict({n: sd[n] for n in own if n in sd}, strict=False)
    return m


@torch.no_grad()
def image_features(m, arrays):
    px = torch.from_numpy(np.stack([fx.clip_preprocess(a) for a in arrays]))
    return m.visual_projection(m.vision_model(pixel_values=px).pooler_output)


@torch.no_grad()
def text_features(m, ids):
    return m.text_projection(m.text_model(input_ids=torch.from_numpy(ids)).pooler_output)


@torch.no_grad()
def e2e(m, tmp):
    from transformers import CLIPTokenizer
    d = fx.write_tokenizer(os.path.join(tmp, "tok"))
    tok = CLIPTokenizer.from_pretrained(os.path.join(d, "tokenizer"), local_files_only=True)
    ids = np.zeros((len(fx.E2E_CAPTIONS), 77), np.int64)
    for i, c in enumerate(fx.E2E_CAPTIONS):
        t = tok(c)["input_ids"]
        ids[i, :len(t)] = t
    tf = text_features(m, ids)
    tf = tf / tf.norm(dim=1, keepdim=True)
    imf = image_features(m, [fx.image_array(h, w, 500 + i) for i, (h, w) in enumerate(fx.E2E_SIZES)])
    imf = imf / imf.norm(dim=1, keepdim=True)
    # stems COCO_val2014_tiny_%012d sort in image-id order, the order of E2E_CAPTIONS
    score = float(m.logit_scale.exp()) * float((tf.double() * imf.double()).sum(1).mean())
    return tf.numpy().astype(np.float32), np.float64(score)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)              # fixed reduction order: the file regenerates bit for bit
    out, report = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for tag in ("tiny", "b32"):
            m = hf_model(tag)
            n_img = 4 if tag == "tiny" else 2
            out[f"{tag}_img"] = image_features(m, fx.model_images(n_img)).numpy().astype(np.float32)
            out[f"{tag}_txt"] = text_features(m, fx.text_ids(tag, n=5 if tag == "tiny" else 3)).numpy().astype(np.float32)
            report.append(f"{tag}: text {fx.CONFIGS[tag][0]} vision {fx.CONFIGS[tag][1]} projection {fx.CONFIGS[tag][2]}")
            report.append(f"  img {out[f'{tag}_img'].shape} max|x| {np.abs(out[f'{tag}_img']).max():.4f}; "
                          f"txt {out[f'{tag}_txt'].shape} max|x| {np.abs(out[f'{tag}_txt']).max():.4f}")
            if tag == "tiny":
                out["e2e_txt"], out["e2e_score"] = e2e(m, tmp)
                report.append(f"  e2e score {float(out['e2e_score']):.6f} over {len(fx.E2E_SIZES)} images")
    import transformers
    report.insert(0, f"transformers {transformers.__version__}, torch {torch.__version__}, fp32 CPU")
    gold = os.path.join(ROOT, "tests", "golden", "clip_score_hf.npz")
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
