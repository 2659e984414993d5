#!/usr/bin/env python3
"""Wall time of one artist of scripts/metrics/artist_erasure.py on one MI355X, per phase: generation (every prompt of the
artist's list, two models, 768 x 768 = 96 x 96 latents, B = 1, 50 PNDM steps, CFG 7.5, bf16, JPEG files written) and scoring
(the files read back, CLIP ViT-B/32 in fp32, pdmk_cosine_pairs).  Random weights throughout (no SD-2.1 or CLIP snapshot is
needed): SD-2.1-shaped student at MAC budget 0.55 with two seeds as "original" and "erased", full-size VAE and text encoder,
ViT-B/32-shaped CLIP.  The tokenizer is the byte-level fixture of tests/data_fixtures.py with its context set to 77 (so the
cross-attention sees SD-2.1's 77 tokens); prompts are cut to 70 characters for it.  The numbers are times, not scores."""
import argparse
import os
import sys
import tempfile
import time

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
from pdm.utils import clip_utils, erasure_utils as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="Monet")
    ap.add_argument("--resolution", type=int, default=768)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--budget", type=float, default=0.55)
    ap.add_argument("--prompts", type=int, default=0, help="first N prompts only (0: all)")
    ap.add_argument("--batch_size", type=int, default=64)
    a = ap.parse_args()
    import data_fixtures as F
    dev = torch.device("cuda:0")
    prompts = [p[:70] for p in E.read_prompts(E.default_prompts_csv(a.target))]
    prompts = prompts[:a.prompts] if a.prompts else prompts
    with tempfile.TemporaryDirectory() as tmp:
        tok = clip_utils.load_tokenizer(F.write_tokenizer(os.path.join(tmp, "tok")))
        tok.model_max_length = 77
        t0 = time.perf_counter()
        cfg = UNetConfig.sd21()
        av, ratio, _ = arch_vector_for_budget(cfg, a.budget, hw=a.resolution // 8)
        unets = [UNet2DConditionModelPruned(cfg, av, dev, torch.bfloat16, train=False, seed=s) for s in (0, 1)]
        vae = AutoencoderKL(None, dev, torch.bfloat16, seed=0)
        txt = CLIPTextModel(None, dev, torch.bfloat16, seed=0)
        pipes = [StableDiffusionPruningPipeline(vae, txt, u, PNDMScheduler(prediction_type="v_prediction"), tok) for u in unets]
        torch.cuda.synchronize()
        t_build = time.perf_counter() - t0
        out = os.path.join(tmp, "concept_erase")
        os.makedirs(out)
        t0 = time.perf_counter()
        E.generate(prompts, out, pipes[0], pipes[1], 0, a.resolution, a.steps)
        torch.cuda.synchronize()
        t_gen = time.perf_counter() - t0
        # a second pass over the first prompts: captured loops and GEMM plans already exist
        warm = os.path.join(tmp, "warm")
        os.makedirs(warm)
        n_warm = min(4, len(prompts))
        t0 = time.perf_counter()
        E.generate(prompts[:n_warm], warm, pipes[0], pipes[1], 0, a.resolution, a.steps)
        torch.cuda.synchronize()
        t_warm = (time.perf_counter() - t0) / (2 * n_warm)
        del pipes, unets, vae, txt
        t0 = time.perf_counter()
        clip = CLIPModel(CLIPTextConfig(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12,
                                        num_attention_heads=8), CLIPVisionConfig(), 512, device=dev, dtype=torch.float32)
        torch.cuda.synchronize()
        t_clip = time.perf_counter() - t0
        t0 = time.perf_counter()
        so, sr, flags = E.score_pairs(prompts, E.pair_files(out, len(prompts)), clip, tok, a.batch_size)
        res = E.statistics(sr.tolist(), flags.tolist())
        t_score = time.perf_counter() - t0
    n = len(prompts)
    print(f"artist_erasure {a.target}: {n} prompts x 2 models, {a.resolution}x{a.resolution}, B=1, {a.steps} PNDM steps, CFG 7.5, "
          f"bf16, budget {ratio:.3f}, random weights")
    print(f"  build (2 students, VAE, text encoder): {t_build:.1f} s")
    print(f"  generation: {t_gen:.1f} s for {2 * n} images = {t_gen / (2 * n):.2f} s/image incl. 2 captures, text encode, VAE decode, "
          f"uint8 rounding, JPEG write; warm {t_warm:.2f} s/image")
    print(f"  CLIP ViT-B/32 (fp32) build: {t_clip:.1f} s")
    print(f"  scoring: {t_score:.2f} s for {n} pairs (JPEG decode, prep, both towers, head; batch {a.batch_size}); "
          f"result {res}")


if __name__ == "__main__":
    main()
