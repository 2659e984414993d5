#!/usr/bin/env python3
"""UCE debiasing (pdm/utils/uce_debias.py) on one MI355X at SD-2.1 shapes, random weights (no snapshot is needed to time
anything): SD-2.1-shaped student at MAC budget 0.55, full-size VAE and text encoder (bf16 compute, fp32 master weights),
ViT-B/32-shaped CLIP (fp32), the byte-level tokenizer of tests/data_fixtures.py with a 77-token context.
  1. `debias_model` on one concept (5 old texts, 2 attributes, the 225-profession retain list): per outer iteration the time of
     sampling, decode + uint8, prep + image tower, head (the stages of get_ratios, a device synchronise at every mark), and of
     the edit split into encode, gram / factor, solve, project, delta, update (the `stages` callback).  The first iteration
     captures the sampler's and the tower's graphs and tunes GEMM plans; the later ones are the steady state.
  2. A same-process A/B of the measurement's classification at the batch `--num_images`: `classify_frames` on the device
     frames against the host route on the same frames (the read-back of output_type="u8_round", pack_images, prep_images,
     encode_image, torch softmax and mask, read back) - warm-up, then alternating repeats timed by device events, medians.
Writes the lines to stdout and to --out.  Nothing is asserted beyond both routes giving the same masks."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unlearn-ft_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pdm.models.clip.clip_model import CLIPModel, CLIPVisionConfig  # noqa: E402
from pdm.models.clip.text_encoder import CLIPTextConfig, CLIPTextModel  # noqa: E402
from pdm.models.unet.spec import UNetConfig, arch_vector_for_budget  # noqa: E402
from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned  # noqa: E402
from pdm.models.vae.autoencoder_kl import AutoencoderKL  # noqa: E402
from pdm.pipelines.pruning_pipelines import PNDMScheduler, StableDiffusionPruningPipeline  # noqa: E402
from pdm.utils import clip_utils, uce_debias as D  # noqa: E402

MEASURE = ("encode_texts", "sample", "decode", "tower", "head")
EDIT = ("encode", "gram_factor", "solve", "project", "delta", "update")


class Clock:
    """callable(name): the time since the previous mark, after a device synchronise, is added to `name`."""

    def __init__(self):
        self.t, self.acc = None, {}

    def start(self):
        torch.cuda.synchronize()
        self.t = time.perf_counter()

    def __call__(self, name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.acc[name] = self.acc.get(name, 0.0) + now - self.t
        self.t = now

    def take(self):
        out, self.acc = self.acc, {}
        return out


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--concept", default="doctor")
    ap.add_argument("--attributes", default="male, female")
    ap.add_argument("--resolution", type=int, default=768)
    ap.add_argument("--num_images", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--budget", type=float, default=0.55)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "debias_bench.txt"))
    a = ap.parse_args()
    import data_fixtures as F
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    settings = dict(D.load_settings(), max_iterations=a.iterations)
    old, new, retain, name = D.build_texts(a.concept, a.attributes, None, "2.1", settings)
    with tempfile.TemporaryDirectory() as tmp:
        tok = clip_utils.load_tokenizer(F.write_tokenizer(os.path.join(tmp, "tok")))
    tok.model_max_length = 77
    cfg = UNetConfig.sd21()
    av, ratio, _ = arch_vector_for_budget(cfg, a.budget, hw=a.resolution // 8)
    unet = UNet2DConditionModelPruned(cfg, av, dev, torch.bfloat16, train=False, seed=0)
    vae = AutoencoderKL(None, dev, torch.bfloat16, seed=0)
    txt = CLIPTextModel(None, dev, torch.bfloat16, seed=0)
    pipe = StableDiffusionPruningPipeline(vae, txt, unet, PNDMScheduler(prediction_type="v_prediction"), tok)
    clip = CLIPModel(CLIPTextConfig(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12,
                                    num_attention_heads=8), CLIPVisionConfig(), 512, device=dev, dtype=torch.float32)
    e = unet.store.by_key["attn2_kv_all.weight"]
    say(f"debias {name}: {len(old)} old texts x {len(new[0])} attributes, {len(retain)} retained texts, {a.resolution}x{a.resolution}, "
        f"num_images {a.num_images}, {settings['num_seeds']} seeds, {settings['num_inference_steps']} PNDM steps, CFG "
        f"{settings['guidance_scale']}, bf16 sampler, budget {ratio:.3f}, attn2_kv_all {tuple(e.shape)}, random weights")

    # ---- 1. the outer loop, stage by stage
    measure, edit = Clock(), Clock()
    per_iteration = []
    inner_ratios, inner_edit = D.get_ratios, D.debias_edit

    def timed_ratios(*args, **kw):
        measure.start()
        out = inner_ratios(*args, **kw)
        measure("read_back")
        per_iteration.append({"measure": measure.take()})
        return out

    def timed_edit(*args, **kw):
        edit.start()
        out = inner_edit(*args, **kw)
        per_iteration[-1]["edit"] = edit.take()
        return out

    D.get_ratios, D.debias_edit = timed_ratios, timed_edit
    try:
        t0 = time.perf_counter()
        weights, init_ratios, ratios, iterations = D.debias_model(
            pipe, clip, tok, old, new, retain, np.random.RandomState(0), num_images=a.num_images, resolution=a.resolution,
            settings=settings, stages=edit, timing=measure)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        D.get_ratios, D.debias_edit = inner_ratios, inner_edit
    say(f"== debias_model: {iterations} measurements in {total:.1f} s; captures {pipe.captures}; ratios {[r.tolist() for r in ratios]}")
    batches = len(old) * int(settings["num_seeds"])
    for i, it in enumerate(per_iteration):
        m = it["measure"]
        say(f"   iteration {i}: measurement {sum(m.values()):8.3f} s over at most {batches} batches of {a.num_images}: " +
            ", ".join(f"{n} {m.get(n, 0.0):.3f}" for n in MEASURE + ("read_back",)))
        if "edit" in it:
            ed = it["edit"]
            say(f"                edit {sum(ed.values()) * 1e3:10.3f} ms: " + ", ".join(f"{n} {ed.get(n, 0.0) * 1e3:.3f}" for n in EDIT))

    # ---- 2. classification of one batch of frames: device-resident against the host route, same frames
    B, R = a.num_images, clip.image_size
    emb = pipe.text_encoder(pipe._tokenize([old[0]]))[0].expand(B, -1, -1)
    neg = pipe.text_encoder(pipe._tokenize([""]))[0].expand(B, -1, -1)
    lat = D.seed_latents(pipe, 1, B, a.resolution).to(dev)
    z = pipe.generate_samples(prompt_embeds=emb, negative_prompt_embeds=neg, latents=lat,
                              num_inference_steps=int(settings["num_inference_steps"]), guidance_scale=7.5, height=a.resolution,
                              width=a.resolution, output_type="latent").images
    frames = D.decode_frames(pipe, z)
    classes = clip.encode_text(clip_utils.tokenize(tok, new[0], context_length=clip.context_length))
    group = torch.zeros(B, dtype=torch.int32, device=dev)
    hits = torch.zeros((1, len(new[0])), device=dev, dtype=torch.int32)
    scale = D.logit_scale(clip)

    def device_route():
        return D.classify_frames(clip, frames, classes, group, hits)[1]

    def host_route():
        host = frames.cpu().numpy()                                  # what output_type="u8_round" hands back
        packed, desc = clip_utils.pack_images(list(host), R)
        img = clip.encode_image(clip_utils.prep_images(packed, desc, R, dev))
        img = img / img.norm(dim=1, keepdim=True)
        t = classes / classes.norm(dim=1, keepdim=True)
        probs = (scale * img @ t.T).softmax(dim=1)
        return probs.ge(probs.max(1, keepdim=True)[0]).float().cpu()

    for _ in range(3):
        md, mh = device_route(), host_route()
    torch.cuda.synchronize()
    same = bool(torch.equal(md.cpu().float(), mh))
    td, th = [], []
    for _ in range(a.repeats):
        td.append(event_ms(device_route)[0])
        th.append(event_ms(host_route)[0])
    d, h = statistics.median(td), statistics.median(th)
    say(f"== classification of {B} frames of {a.resolution}x{a.resolution}, median of {a.repeats} alternating repeats (device events), "
        f"masks equal: {same}")
    say(f"   classify_frames (device frames, no read-back): {d:8.3f} ms   [{min(td):.3f} .. {max(td):.3f}]")
    say(f"   host route (read-back, pack, H2D, prep, tower, torch softmax, read-back): {h:8.3f} ms   [{min(th):.3f} .. {max(th):.3f}]")
    say(f"   host / device = {h / d:.2f}")
    with open(a.out, "w") as f:
        f.write("# tools/debias_bench.py on 1 x MI355X; command: python tools/debias_bench.py\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
