"""pdm/utils/load_models.py on the GPU (-m gpu), on the shared tiny tree of data_fixtures.write_pruned_checkpoint_tree: the
student comes back bit for bit, the frozen models are built once, a missing VAE is an error without random_init, and the
trainer reads the same objects through its `models`."""
import os

import pytest
import torch

import data_fixtures

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tree(tmp_path_factory, dev):
    return data_fixtures.write_pruned_checkpoint_tree(str(tmp_path_factory.mktemp("load_models")), dev, "lm.yaml")


def test_load_unet_returns_the_saved_weights(dev, tree):
    from pdm.utils.load_models import FrozenModels, inference_config
    models = FrozenModels(inference_config(tree["yaml"], tree["snap"], tiny=True), dev)
    unet = models.load_unet(tree["ck"])
    assert unet.dtype == torch.float32 and not unet.training
    sd = unet.state_dict()
    assert list(sd) == list(tree["sd"])
    for n, v in tree["sd"].items():
        assert sd[n].dtype == v.dtype and torch.equal(sd[n].contiguous().view(torch.int32), v.contiguous().view(torch.int32)), n


def test_frozen_models_are_built_once_and_shared_by_pipelines(dev, tree):
    from pdm.pipelines.pruning_pipelines import DDIMScheduler, PNDMScheduler
    from pdm.utils.load_models import FrozenModels, inference_config
    models = FrozenModels(inference_config(tree["yaml"], tree["snap"], tiny=True), dev)
    vae, enc, tok = models.vae, models.text_encoder, models.tokenizer
    assert models.vae is vae and models.text_encoder is enc and models.tokenizer is tok
    unet = models.load_unet(tree["ck"])
    a, b = models.pipeline(unet), models.pipeline(unet, "ddim")
    assert type(a.scheduler) is PNDMScheduler and type(b.scheduler) is DDIMScheduler and a.scheduler is not b.scheduler
    assert a.scheduler.config.prediction_type == b.scheduler.config.prediction_type == "v_prediction"
    for p in (a, b):
        assert p.vae is vae and p.text_encoder is enc and p.tokenizer is tok and p.unet is unet


def test_missing_vae_is_an_error_without_random_init(dev, tree):
    from pdm.utils.config import load_config
    from pdm.utils.load_models import FrozenModels
    config = load_config(tree["yaml"])
    config.model.prediction_model.random_init = False
    models = FrozenModels(config, dev)
    assert not os.path.isdir(os.path.join(tree["snap"], "vae"))
    with pytest.raises(FileNotFoundError, match="VAE: .*snapshot/vae' is not a local directory"):
        models.vae
    with pytest.raises(FileNotFoundError, match="text encoder: "):
        models.text_encoder


def test_trainer_delegates_to_its_models(dev, tree, tmp_path):
    from pdm.training.trainer import UnetFineTuner
    from pdm.utils.config import load_config
    config = load_config(tree["yaml"])
    config.update({"synthetic": True, "pruning_ckpt_dir": tree["ck"], "logging_dir": str(tmp_path / "logs"),
                   "data": {"dataloader": {"train_batch_size": 1}}})
    tr = UnetFineTuner(config)
    assert tr._empty_cache == {}
    assert tr.vae is tr.models.vae and tr.text_encoder is tr.models.text_encoder and tr.tokenizer is tr.models.tokenizer
    assert tr.weight_dtype is tr.models.weight_dtype and tr.weight_dtype == torch.float32
    assert tr.unet_config is tr.models.unet_config
    pipe = tr.get_pipeline()
    assert pipe.vae is tr.vae and pipe.text_encoder is tr.text_encoder and pipe.unet is tr.prediction_model
    assert pipe.tokenizer is None and pipe.scheduler.config.prediction_type == "v_prediction"
