"""The trainers on real (local) data: a tiny COCO tree and an upper `datasets` directory with a `style` column, read by
pdm/utils/data.py, decoded by the DataLoader workers and preprocessed by pdmk_image_prep - no `synthetic` anywhere."""
import importlib.util
import json
import os

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")

import numpy as np
import pytest
import torch

import data_fixtures as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree(tmp_path, upper_caption="prompt"):
    """snapshot/tokenizer, coco/, upper/ and a pruning checkpoint (quantizer_embeddings.pt, trainer.py:2159-2161)."""
    from pdm_ref import arch as oarch
    from pdm_ref.config import UNetConfig as OCfg
    root = str(tmp_path)
    snap = F.write_tokenizer(os.path.join(root, "snapshot"))
    coco = F.write_coco(root, "2017", n=10)
    upper = F.write_style_dataset(root, n=8, caption_column=upper_caption)
    ck = os.path.join(root, "pruning")
    os.makedirs(ck)
    ocfg = OCfg.tiny()
    torch.save(torch.stack([oarch.random_arch_vector(ocfg, kr, seed=s)[0] for s, kr in ((1, 0.6), (2, 0.8))]),
               os.path.join(ck, "quantizer_embeddings.pt"))
    return snap, coco, upper, ck


def _config(tmp_path, steps, hip_graphs=False, workers=2):
    from pdm.utils.config import Cfg
    snap, coco, upper, ck = _tree(tmp_path)
    return Cfg.wrap({
        "seed": 43, "tiny": True, "mixed_precision": "bf16", "pretrained_model_name_or_path": snap,
        "pruning_ckpt_dir": ck, "expert_id": 1,
        "model": {"prediction_model": {"prediction_type": "v_prediction", "resolution": 128, "gated_ff": True,
                                       "ff_gate_width": 32, "random_init": True}},
        "data": {"data_dir": coco, "year": 2017, "prompts": ["the red square", "a blue and green thing"],
                 "dataloader": {"train_batch_size": 2, "dataloader_num_workers": workers, "random_flip": True,
                                "center_crop": False, "image_generation_batch_size": 2}},
        "upper_data": {"dataset_name": upper, "caption_column": "prompt", "style": "monet"},
        "training": {"max_train_steps": steps, "upper_step_freq": 3, "hip_graphs": hip_graphs,
                     "losses": {"diffusion_loss": {"snr_gamma": 5.0, "weight": 1.0},
                                "distillation_loss": {"weight": 2.0, "upper_weight": 1.0},
                                "block_loss": {"weight": 0.1, "upper_weight": 0.0}},
                     "optim": {"prediction_model_learning_rate": 1e-4, "prediction_model_upper_learning_rate": 5e-4,
                               "lr_warmup_steps": 2},
                     "logging": {"logging_dir": str(tmp_path / "logs"), "checkpoint_steps": 4}}})


def _reference_pixels(path, desc, R):
    """The reference's transform on the loader's recorded draws: PIL resize -> crop -> flip -> ToTensor -> Normalize."""
    from PIL import Image
    off, h, w, rh, rw, top, left, flip = desc
    with Image.open(path) as im:
        img = im.convert("RGB")
    assert (img.height, img.width) == (h, w)
    r = img.resize((rw, rh), Image.BILINEAR) if (rh, rw) != (h, w) else img
    r = r.crop((left, top, left + R, top + R))
    if flip:
        r = r.transpose(Image.FLIP_LEFT_RIGHT)
    x = torch.from_numpy(np.array(r, np.uint8, copy=True)).permute(2, 0, 1).contiguous().float().div(255)
    return x.sub(0.5).div(0.5)


def test_bilevel_trainer_trains_on_local_data(dev, tmp_path):
    from pdm.training.trainer import BilevelUnetFineTuner
    from transformers import CLIPTokenizer
    tr = BilevelUnetFineTuner(_config(tmp_path, 6))
    assert torch.equal(tr.arch_vector, torch.load(str(tmp_path / "pruning" / "quantizer_embeddings.pt"))[1][None])
    assert len(tr.train_dataloader) == 10 and len(tr.upper_dataloader) == 2         # 20 captions; 4 "monet" rows, bs 2
    w0 = tr.prediction_model.store.master.clone()
    tr.train()
    assert tr.global_step == 6 and not torch.equal(w0, tr.prediction_model.store.master)
    recs = [json.loads(l) for l in open(tmp_path / "logs" / "metrics.jsonl")]
    assert len(recs) == 6 and [r["step"] for r in recs if "finetuning/upper_loss" in r] == [2, 5]
    for r in recs:
        assert all(np.isfinite(v) for k, v in r.items() if k.startswith("finetuning/")), r
    for ck in ("checkpoint-4", "checkpoint-6"):
        assert (tmp_path / "logs" / ck / "unet" / "diffusion_pytorch_model.safetensors").exists()
        assert (tmp_path / "logs" / ck / "optimizer_1.bin").exists()
    # a batch of the next epoch: pixel values equal the reference transform for the recorded crop / flip draws, token ids
    # equal CLIPTokenizer on the chosen captions
    R = 128 // 8 * tr.vae_factor
    tok = CLIPTokenizer.from_pretrained(str(tmp_path / "snapshot"), subfolder="tokenizer", local_files_only=True)
    rows = tr.train_dataloader.rows
    flips = 0
    for k, batch in enumerate(tr.train_dataloader):
        assert batch["pixel_values"].shape == (2, 3, R, R) and batch["pixel_values"].device.type == "cuda"
        px = batch["pixel_values"].cpu()
        for j, i in enumerate(batch["index"].tolist()):
            desc = batch["image_desc"][j].tolist()
            flips += desc[7]
            assert (px[j] - _reference_pixels(rows[i]["image"], desc, R)).abs().max().item() == 0.0, (k, j, desc)
        want = tok(batch["captions"], padding="max_length", max_length=tok.model_max_length, truncation=True,
                   return_tensors="pt").input_ids
        assert torch.equal(batch["input_ids"].cpu(), want) and want.shape == (2, F.T)
        assert torch.equal(batch["empty_input_ids"].cpu(), tok(["", ""], padding="max_length", max_length=F.T, truncation=True,
                                                               return_tensors="pt").input_ids)
    assert 0 < flips < 20
    # the upper loader holds the "monet" rows only; the prompt loader tokenises data.prompts
    ub = next(iter(tr.upper_dataloader))
    up_rows = tr.upper_dataloader.rows
    assert set(up_rows["style"]) == {"monet"} and ub["pixel_values"].shape == (2, 3, R, R)
    pb = next(iter(tr.prompt_dataloader))
    assert pb["input_ids"].shape == (2, F.T) and pb["prompts"] == ["the red square", "a blue and green thing"]


def test_hip_graph_mode_trains_like_eager_mode_on_local_data(dev, tmp_path):
    """Same data, same seeds: graph replay gives the eager loss curve (tolerance of test_hip_graph_mode_trains_like_eager_mode)."""
    from pdm.training.trainer import BilevelUnetFineTuner
    runs = []
    for name, mode in (("e", False), ("g", True)):
        cfg = _config(tmp_path / name, 6, hip_graphs=mode, workers=0 if mode else 2)
        tr = BilevelUnetFineTuner(cfg)
        tr.train()
        runs.append(([json.loads(l) for l in open(tmp_path / name / "logs" / "metrics.jsonl")],
                     tr.prediction_model.store.master.clone()))
    (re, we), (rg, wg) = runs
    assert len(re) == len(rg) == 6 and [sorted(r) for r in re] == [sorted(r) for r in rg]
    for a, b in zip(re, rg):
        for key in a:
            assert abs(a[key] - b[key]) <= 2e-2 * abs(a[key]) + 1e-7, (key, a[key], b[key])
    d = (we - wg).abs()
    assert d.max().item() <= 5e-3 and d.mean().item() <= 2e-3 * we.abs().mean().item() + 1e-6


def test_bilevel_entry_script_runs_the_reference_yaml_on_local_data(dev, tmp_path, monkeypatch):
    """scripts/aptp/bilevel_finetune.py::main() over the reference's key tree with `data.data_dir` set, a local pruning
    checkpoint and a local snapshot (tokenizer only; random_init for the weights) - no --synthetic."""
    import sys
    import test_entry_scripts_gpu as E
    snap, coco, _, ck = _tree(tmp_path)
    upper = F.write_style_dataset(str(tmp_path / "u2"), n=6, styles=("Claude Monet", "other"), caption_column="caption")
    text = (E.YAML.replace('data_dir: "/path/to/dataset"', f'data_dir: "{coco}"')
            .replace('dataset_name: "rezashkv/controlled_distillation"', f'dataset_name: "{upper}"')
            .replace("gated_ff: true", "gated_ff: true\n    random_init: true")
            .replace("@LOGDIR@", str(tmp_path / "logs")))
    assert f'data_dir: "{coco}"' in text and f'dataset_name: "{upper}"' in text and "random_init: true" in text
    path = tmp_path / "recipe.yaml"
    path.write_text(text)
    spec = importlib.util.spec_from_file_location("entry_bilevel_data", os.path.join(ROOT, "unlearn-ft_amd", "scripts", "aptp",
                                                                                     "bilevel_finetune.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["bilevel_finetune.py", "--base_config_path", str(path), "--pruning_ckpt_dir", ck,
                                      "--expert_id", "0", "--tiny", "--mixed_precision", "bf16",
                                      "--pretrained_model_name_or_path", snap])
    mod.main()
    recs = [json.loads(l) for l in open(tmp_path / "logs" / "metrics.jsonl")]
    assert len(recs) == 3 and all(np.isfinite(r["finetuning/loss"]) for r in recs)
    assert [r["step"] for r in recs if "finetuning/upper_loss" in r] == [1]
    assert (tmp_path / "logs" / "checkpoint-3" / "arch_vector.pt").exists()
    assert (tmp_path / "logs" / "images" / "step-0.npy").exists()              # image logging over data.prompts
