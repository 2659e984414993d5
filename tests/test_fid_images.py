"""scripts/metrics/generate_fid_images.py host logic (no GPU): row sharding over ranks, output names, the PNDM scheduler
config."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location(
        "fid_images_host", os.path.join(ROOT, "unlearn-ft_amd", "scripts", "metrics", "generate_fid_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 5, 7, 10, 13])
def test_every_row_once_rank_r_takes_batches_r_plus_kw(world, n):
    m = _script()
    per = 2
    batch = per * world
    seen = []
    for r in range(world):
        got = m.rank_batches(n, batch, world, r)
        starts = [b[0] // batch for b in got]
        assert starts == list(range(r, (n + batch - 1) // batch, world))          # batches r, r + W, ...
        for b in got:
            assert b == list(range(b[0], min(b[0] + batch, n)))                      # consecutive rows, no padding
        seen += [i for b in got for i in b]
    assert sorted(seen) == list(range(n))


def test_names_and_output_dir(tmp_path):
    from pdm.utils.config import Cfg
    m = _script()
    assert m.image_file_name("/data/coco/images/val2014/COCO_val2014_000000000042.jpg") == "COCO_val2014_000000000042.npy"
    assert m.image_file_name("x/y/photo.png") == "photo.png.npy"
    assert m.image_file_name("x/y/photo.jpeg") == "photo.jpeg.npy"
    assert m.image_file_name({"path": "a/b/c.jpg", "bytes": None}) == "c.npy"
    cfg = Cfg.wrap({"finetuning_ckpt_dir": str(tmp_path), "data": {"data_dir": "/x/coco"},
                    "training": {"num_inference_steps": 10}})
    assert m.output_dir(cfg) == os.path.join(str(tmp_path), "None_fid_images_10")


SD21 = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.8.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
        "beta_start": 0.00085, "clip_sample": False, "num_train_timesteps": 1000, "prediction_type": "v_prediction",
        "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None}


def test_scheduler_config_loaded_and_unsupported_values_raise(tmp_path):
    import torch
    from pdm.pipelines.pruning_pipelines import PNDMScheduler
    from pdm.utils.config import Cfg
    from pdm.utils.load_models import load_scheduler
    d = tmp_path / "snap" / "scheduler"
    d.mkdir(parents=True)
    (d / "scheduler_config.json").write_text(json.dumps({**SD21, "num_train_timesteps": 500, "steps_offset": 0}))
    s = load_scheduler(Cfg.wrap({"pretrained_model_name_or_path": str(tmp_path / "snap")}))
    assert s.config.prediction_type == "v_prediction" and s.config.num_train_timesteps == 500 and s.config.steps_offset == 0
    assert torch.equal(s.alphas_cumprod, PNDMScheduler(num_train_timesteps=500).alphas_cumprod)
    s.set_timesteps(10)
    assert s.timesteps.tolist()[:3] == [450, 400, 400]
    # no file: SD-2.1 defaults with the config's prediction type
    s = load_scheduler(Cfg.wrap({"pretrained_model_name_or_path": str(tmp_path / "none"),
                                 "model": {"prediction_model": {"prediction_type": "epsilon"}}}))
    assert s.config.prediction_type == "epsilon" and s.config.steps_offset == 1
    for bad in ({"skip_prk_steps": False}, {"beta_schedule": "linear"}, {"set_alpha_to_one": True},
                {"prediction_type": "sample"}, {"trained_betas": [0.1]}, {"some_new_option": 1}):
        with pytest.raises(ValueError):
            PNDMScheduler.from_config({**SD21, **bad})


def test_plms_rows_follow_step():
    """The step table: modes, history slots and coefficients of PNDMScheduler.step for every index."""
    from pdm.pipelines.pruning_pipelines import PNDMScheduler
    s = PNDMScheduler(prediction_type="v_prediction")
    s.set_timesteps(10)
    rows = s.plms_rows()
    assert [r.t for r in rows] == s.timesteps.tolist() and len(rows) == 11
    assert [r.mode for r in rows] == [0, 1] + [2] * 9
    assert [r.wslot for r in rows] == [0, -1, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    assert [r.nterms for r in rows[2:]] == [2, 3, 4, 4, 4, 4, 4, 4, 4]
    assert rows[1].rslot[0] == 0 and list(rows[1].coef[:2]) == [0.5, 0.5]
    assert list(rows[5].rslot) == [3, 2, 1] and rows[5].coef[0] == pytest.approx(55 / 24)
    assert all(r.vpred == 1 for r in rows)
