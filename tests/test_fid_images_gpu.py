"""scripts/metrics/generate_fid_images.py end to end (-m gpu): train 2 steps on a fixture COCO tree whose `val` split has an
image with two captions, then generate the FID images from `checkpoint-2` - captured, eager (PDMK_SAMPLER_GRAPH=0) and on
two ranks sharing the GPU."""
import importlib.util
import json
import os
import socket
import subprocess
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")

import numpy as np
import pytest
import torch
import yaml

import data_fixtures as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "unlearn-ft_amd", "scripts", "metrics", "generate_fid_images.py")
VAL = [(1, "a red thing"), (2, "the blue one"), (3, "first caption of three"), (3, "second caption of three"),
       (4, "and the fourth"), (5, "of the fifth")]          # image 3 has two captions: rows 2 and 3


def _script():
    spec = importlib.util.spec_from_file_location("fid_images_gpu", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_val(coco):
    """<coco>/images/val2017 + annotations/captions_val2017.json with the rows of VAL, in that order."""
    d = os.path.join(coco, "images", "val2017")
    os.makedirs(d, exist_ok=True)
    for i in sorted({i for i, _ in VAL}):
        F.image(40, 48, seed=50 + i).save(os.path.join(d, "%012d.jpg" % i), quality=90)
    ann = [{"image_id": i, "id": 100 + j, "caption": c} for j, (i, c) in enumerate(VAL)]
    with open(os.path.join(coco, "annotations", "captions_val2017.json"), "w") as f:
        json.dump({"annotations": ann}, f)


def _setup(tmp_path, bs):
    """Fixture tree, a 2-step training run (checkpoint-2) and the YAML the script reads."""
    from pdm.training.trainer import UnetFineTuner
    from pdm.utils.config import Cfg
    root = str(tmp_path)
    snap = F.write_tokenizer(os.path.join(root, "snapshot"))
    coco = F.write_coco(root, "2017", n=4)
    _write_val(coco)
    cfg = {"seed": 43, "tiny": True, "pretrained_model_name_or_path": snap,
           "model": {"prediction_model": {"prediction_type": "v_prediction", "resolution": 128, "gated_ff": True,
                                          "ff_gate_width": 32, "random_init": True}},
           "data": {"data_dir": coco, "year": 2017,
                    "dataloader": {"train_batch_size": 2, "dataloader_num_workers": 0, "image_generation_batch_size": bs}},
           "training": {"max_train_steps": 2, "num_inference_steps": 3, "mixed_precision": "bf16",
                        "optim": {"prediction_model_learning_rate": 1e-4},
                        "logging": {"logging_dir": os.path.join(root, "logs"), "checkpoint_steps": 2}}}
    UnetFineTuner(Cfg.wrap(cfg)).train()
    path = os.path.join(root, "fid.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path, os.path.join(root, "logs", "checkpoint-2"), snap


def _argv(path, ck, snap):
    return ["generate_fid_images.py", "--base_config_path", path, "--finetuning_ckpt_dir", ck, "--tiny",
            "--pretrained_model_name_or_path", snap, "--image_resolution", "64", "--seed", "43"]


def _expected(m, argv, batches, dev):
    """{row: uint8 image} of the eager pipeline over the given batches of rows (numpy truncation of its float output)."""
    from pdm.utils.arg_utils import parse_args
    from pdm.utils.config import load_config
    from pdm.utils.load_models import FrozenModels
    args = parse_args(argv[1:])
    config = load_config(args.base_config_path)
    config.update(vars(args))
    models = FrozenModels(config, dev)
    pipe = models.pipeline(models.load_unet(config.finetuning_ckpt_dir))
    caps, _ = m.validation_rows(config)
    out = {}
    for rows in batches:
        gen = torch.Generator(device=dev).manual_seed(43)
        f = pipe(prompt=[caps[i] for i in rows], num_inference_steps=3, generator=gen, output_type="np", height=64, width=64,
                 graph=False).images
        out.update({i: (img * 255).astype(np.uint8) for i, img in zip(rows, f)})
    return out


def _files(out):
    return {n: np.load(os.path.join(out, n)) for n in sorted(os.listdir(out))}


def test_generate_fid_images_end_to_end(dev, tmp_path, monkeypatch):
    m = _script()
    path, ck, snap = _setup(tmp_path, bs=4)
    argv = _argv(path, ck, snap)
    monkeypatch.setattr(sys, "argv", argv)
    m.main()
    out = os.path.join(ck, "None_fid_images_3")
    got = _files(out)
    assert sorted(got) == ["%012d.npy" % i for i in (1, 2, 3, 4, 5)]
    for a in got.values():
        assert a.shape == (64, 64, 3) and a.dtype == np.uint8
    want = _expected(m, argv, m.rank_batches(len(VAL), 4, 1, 0), dev)         # batches of 4 and 2 rows: the last one short
    for row, (i, _) in enumerate(VAL):
        if row == 2:
            continue                                                            # overwritten by row 3 (same image)
        assert np.array_equal(got["%012d.npy" % i], want[row]), row
    assert not np.array_equal(want[2], want[3])
    # the eager loop writes the same bytes
    before = {n: open(os.path.join(out, n), "rb").read() for n in got}
    monkeypatch.setenv("PDMK_SAMPLER_GRAPH", "0")
    m.main()
    assert {n: open(os.path.join(out, n), "rb").read() for n in got} == before


def test_generate_fid_images_two_ranks_one_gpu(dev, tmp_path):
    """Each rank's files equal what one process computes for that rank's batches.  The ranks import this process's GEMM
    plans (PDMK_PLAN_CACHE), so that all three launch the same kernels."""
    from pdm import _pdmk as k
    m = _script()
    path, ck, snap = _setup(tmp_path, bs=1)
    argv = _argv(path, ck, snap)
    # batches of 1 x 2 rows: rank 0 takes rows 0, 1, 4, 5, rank 1 rows 2, 3
    want = [(m.rank_batches(len(VAL), 2, 2, r), _expected(m, argv, m.rank_batches(len(VAL), 2, 2, r), dev)) for r in range(2)]
    plans = str(tmp_path / "plans.txt")
    k.plan_export(plans)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {**os.environ, "WORLD_SIZE": "2", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
           "PDMK_PLAN_CACHE": plans}
    procs = [subprocess.Popen([sys.executable, SCRIPT] + argv[1:], env={**env, "RANK": str(r)}, cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    out = os.path.join(ck, "None_fid_images_3")
    got = _files(out)
    assert sorted(got) == ["%012d.npy" % i for i in (1, 2, 3, 4, 5)]
    for r, (batches, rows_want) in enumerate(want):
        for rows in batches:
            for row in rows:
                if row == 2:
                    continue                                        # overwritten by row 3 (same image, same batch)
                assert np.array_equal(got["%012d.npy" % VAL[row][0]], rows_want[row]), (r, row)
