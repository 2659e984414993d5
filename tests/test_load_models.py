"""pdm/utils/load_models.py host logic (no GPU): the scheduler file-or-defaults rule for both classes, the script config, the
weight dtype rule and the U-Net keyword set; and the one scheduler base's per-class key tables."""
import json

import pytest
import torch
import yaml

from pdm.pipelines.pruning_pipelines import DDIMScheduler, PNDMScheduler
from pdm.utils import load_models as LM
from pdm.utils.config import Cfg

SD21 = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.8.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
        "beta_start": 0.00085, "clip_sample": False, "num_train_timesteps": 1000, "prediction_type": "v_prediction",
        "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None}


@pytest.mark.parametrize("kind,cls", [("pndm", PNDMScheduler), ("ddim", DDIMScheduler)])
def test_load_scheduler_reads_the_snapshot_file_or_takes_the_defaults(tmp_path, kind, cls):
    d = tmp_path / "snap" / "scheduler"
    d.mkdir(parents=True)
    (d / "scheduler_config.json").write_text(json.dumps({**SD21, "num_train_timesteps": 500, "steps_offset": 0}))
    s = LM.load_scheduler(Cfg.wrap({"pretrained_model_name_or_path": str(tmp_path / "snap")}), kind)
    assert type(s) is cls
    assert s.config.prediction_type == "v_prediction" and s.config.num_train_timesteps == 500 and s.config.steps_offset == 0
    assert torch.equal(s.alphas_cumprod, cls(num_train_timesteps=500).alphas_cumprod)
    s.set_timesteps(10)
    assert s.timesteps.tolist()[:3] == ([450, 400, 400] if kind == "pndm" else [450, 400, 350])
    # no file: SD-2.1 defaults with the config's prediction type
    s = LM.load_scheduler(Cfg.wrap({"pretrained_model_name_or_path": str(tmp_path / "none"),
                                    "model": {"prediction_model": {"prediction_type": "epsilon"}}}), kind)
    assert type(s) is cls
    assert s.config.prediction_type == "epsilon" and s.config.steps_offset == 1 and s.config.num_train_timesteps == 1000
    assert LM.load_scheduler(Cfg(), kind).config.prediction_type == "v_prediction"
    assert type(LM.load_scheduler(Cfg())) is PNDMScheduler


def test_one_file_serves_both_classes_with_their_own_tables():
    assert PNDMScheduler.from_config(SD21).config.skip_prk_steps is True
    assert not hasattr(DDIMScheduler.from_config(SD21).config, "skip_prk_steps")
    with pytest.raises(ValueError, match="PNDMScheduler.*thresholding"):       # a key only DDIM knows
        PNDMScheduler.from_config({**SD21, "thresholding": False})
    DDIMScheduler.from_config({**SD21, "thresholding": False})
    with pytest.raises(ValueError, match="PNDMScheduler.*skip_prk_steps"):
        PNDMScheduler.from_config({**SD21, "skip_prk_steps": False})
    DDIMScheduler.from_config({**SD21, "skip_prk_steps": False})                # ignored: PNDM's key
    with pytest.raises(ValueError, match="DDIMScheduler.*thresholding"):
        DDIMScheduler.from_config({**SD21, "thresholding": True})


@pytest.mark.parametrize("cls", [PNDMScheduler, DDIMScheduler])
def test_unsupported_prediction_type_raises_at_construction(cls):
    with pytest.raises(ValueError, match=cls.__name__ + ".*prediction_type"):
        cls(prediction_type="sample")


def test_inference_config(tmp_path):
    c = LM.inference_config(None)
    assert dict(c) == {"tiny": False}
    assert dict(LM.inference_config(None, "snap", True, "bf16")) == {"tiny": True, "pretrained_model_name_or_path": "snap",
                                                                     "mixed_precision": "bf16"}
    path = str(tmp_path / "base.yaml")
    with open(path, "w") as f:
        yaml.safe_dump({"seed": 7, "tiny": False, "pretrained_model_name_or_path": "/yaml/snapshot", "mixed_precision": "bf16",
                        "model": {"prediction_model": {"prediction_type": "epsilon"}}}, f)
    c = LM.inference_config(path, "/flag/snapshot", True, "no")
    assert c.pretrained_model_name_or_path == "/flag/snapshot" and c.tiny is True and c.mixed_precision == "no"
    assert c.seed == 7 and c.get_path("model.prediction_model.prediction_type") == "epsilon"
    c = LM.inference_config(path)                                               # no flags: the YAML's values stay
    assert c.pretrained_model_name_or_path == "/yaml/snapshot" and c.mixed_precision == "bf16" and c.tiny is False
    # train_erase.py: no --model_id keeps the YAML's snapshot, fp32 is forced over the YAML's bf16
    c = LM.inference_config(path, None, True, mixed_precision="no")
    assert c.pretrained_model_name_or_path == "/yaml/snapshot" and c.mixed_precision == "no" and c.tiny is True
    assert LM.FrozenModels(c, None).weight_dtype == torch.float32


def test_weight_dtype_and_topology():
    from pdm.models.unet.spec import UNetConfig
    for mp, want in ((None, torch.float32), ("no", torch.float32), ("bf16", torch.bfloat16)):
        assert LM.FrozenModels(Cfg.wrap({"mixed_precision": mp}), None).weight_dtype == want
        assert LM.FrozenModels(Cfg.wrap({"training": {"mixed_precision": mp}}), None).weight_dtype == want
    assert LM.FrozenModels(Cfg.wrap({"mixed_precision": "no", "training": {"mixed_precision": "bf16"}}), None).weight_dtype == torch.float32
    with pytest.raises(ValueError, match="mixed_precision='fp16' is not supported on this build"):
        LM.FrozenModels(Cfg.wrap({"mixed_precision": "fp16"}), None)
    assert LM.FrozenModels(Cfg.wrap({"tiny": True}), None).unet_config == UNetConfig.tiny()
    assert LM.FrozenModels(Cfg(), None).unet_config == UNetConfig.sd21()


def test_unet_kwargs():
    keys = {"down_block_types", "up_block_types", "mid_block_type", "attention_precision", "gated_ff", "ff_gate_width"}
    kw = LM.unet_kwargs(Cfg.wrap({"attention_precision": "fp32", "model": {"prediction_model": {"prediction_type": "epsilon"}}}))
    assert set(kw) == keys
    assert kw == dict(down_block_types=None, up_block_types=None, mid_block_type=None, attention_precision=None, gated_ff=True,
                      ff_gate_width=32)                                         # the root-level attention_precision is the trainer's
    assert LM.unet_kwargs(Cfg()) == kw
    pm = {"unet_down_blocks": ["CrossAttnDownBlock2DHalfGated", "DownBlock2DHalfGated"], "unet_up_blocks": ["UpBlock2DHalfGated"],
          "unet_mid_block": "UNetMidBlock2DCrossAttnWidthGated", "attention_precision": "bf16", "gated_ff": False, "ff_gate_width": 16}
    kw = LM.unet_kwargs(Cfg.wrap({"attention_precision": "fp32", "model": {"prediction_model": pm}}))
    assert kw == dict(down_block_types=pm["unet_down_blocks"], up_block_types=pm["unet_up_blocks"],
                      mid_block_type=pm["unet_mid_block"], attention_precision="bf16", gated_ff=False, ff_gate_width=16)


def test_golden_path_finds_the_shipped_lists():
    import os
    assert os.path.isfile(LM.golden_path("uce", "artists1734.txt"))
    assert os.path.isfile(os.path.join(LM.golden_path("concept_prune"), "things.txt"))
