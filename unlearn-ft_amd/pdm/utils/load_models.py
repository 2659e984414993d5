"""From a config to inference models (the reference's utils/load_models.py): the one place where the trainer, the evaluation
scripts and the baselines get the frozen VAE / CLIP text encoder / tokenizer of a snapshot, the pruned student of a checkpoint
directory, the sampling scheduler and the pipeline over them.

`FrozenModels(config, device)` holds the dtype and topology rules and builds each frozen model on first use; the trainer owns
one (`Trainer.models`), a script builds its own from `inference_config(...)`.  Nothing here trains, and nothing here touches the
GPU before a model is asked for.
"""
import json
import os

import torch

from .config import Cfg, cfg_get, load_config


def golden_path(*parts):
    """A shipped data file (word lists, prompt tables): <repository>/tests/golden/<parts>."""
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    return os.path.join(root, "tests", "golden", *parts)


def inference_config(base_config_path, model_id=None, tiny=False, mixed_precision=None):
    """The config of an evaluation / baseline script: the YAML (none: empty) with the script's flags laid over its root.
    model_id / mixed_precision None leave the YAML's `pretrained_model_name_or_path` / precision alone."""
    config = load_config(base_config_path) if base_config_path else Cfg()
    config.update({"tiny": tiny})
    if model_id is not None:
        config.update({"pretrained_model_name_or_path": model_id})
    if mixed_precision is not None:
        config.update({"mixed_precision": mixed_precision})
    return config


def cuda_device(index):
    device = torch.device("cuda", int(index))
    torch.cuda.set_device(device)
    return device


def unet_kwargs(config):
    """The `model.prediction_model` keywords of UNet2DConditionModelPruned.from_pretrained."""
    pm = cfg_get(config, "model.prediction_model", {})
    return dict(down_block_types=pm.get("unet_down_blocks"), up_block_types=pm.get("unet_up_blocks"),
                mid_block_type=pm.get("unet_mid_block"), attention_precision=pm.get("attention_precision"),
                gated_ff=pm.get("gated_ff", True), ff_gate_width=pm.get("ff_gate_width", 32))


def load_scheduler(config, kind="pndm"):
    """`kind` "pndm" / "ddim" from <snapshot>/scheduler/scheduler_config.json when present (values the class does not
    implement raise), else the SD-2.1 defaults with `model.prediction_model.prediction_type`.  `kind` "lms" (the UCE
    evaluation scripts build their LMSDiscreteScheduler by hand beside the snapshot's models): the snapshot's file names
    another scheduler class, so only its prediction_type and beta keys are taken and the other class's keys are ignored."""
    from ..pipelines.pruning_pipelines import DDIMScheduler, LMSDiscreteScheduler, PNDMScheduler
    cls = {"pndm": PNDMScheduler, "ddim": DDIMScheduler, "lms": LMSDiscreteScheduler}[kind]
    root = cfg_get(config, "pretrained_model_name_or_path")
    path = os.path.join(str(root), "scheduler", "scheduler_config.json")
    if root and os.path.exists(path):
        if kind == "lms":
            with open(path) as f:
                file = json.load(f)
            return cls(**{key: file[key] for key in ("prediction_type", "beta_start", "beta_end", "num_train_timesteps")
                          if key in file})
        return cls.from_config(path)
    return cls(prediction_type=cfg_get(config, "model.prediction_model.prediction_type", "v_prediction"))


class FrozenModels:
    """Weight dtype, U-Net topology and the frozen VAE / text encoder / tokenizer of `pretrained_model_name_or_path`, each
    built on first use and kept."""

    def __init__(self, config, device):
        from ..models.unet.spec import UNetConfig
        self.config, self.device = config, device
        # trainer.py:516-527: student master weights fp32; bf16 compute under mixed precision
        mp = cfg_get(config, "mixed_precision", None) or cfg_get(config, "training.mixed_precision", None)
        self.weight_dtype = {"bf16": torch.bfloat16, "no": torch.float32, None: torch.float32}.get(mp)
        if self.weight_dtype is None:
            raise ValueError(f"mixed_precision={mp!r} is not supported on this build (use bf16 or no)")
        self.unet_config = UNetConfig.tiny() if cfg_get(config, "tiny", False) else UNetConfig.sd21()
        self._vae = self._text_encoder = self._tokenizer = None

    def allow_random(self, what, path):
        """Random weights / a random arch vector stand in for missing files only when asked for (`--synthetic`, or
        `model.prediction_model.random_init` like the reference's random_init path, unet_2d_conditional.py:2406-2408).
        Otherwise a missing checkpoint is an error, as in the reference (every from_pretrained there raises)."""
        if bool(cfg_get(self.config, "synthetic", False)) or bool(cfg_get(self.config, "model.prediction_model.random_init", False)):
            return True
        raise FileNotFoundError(
            f"{what}: {path!r} is not a local directory / file (hub downloads are not available to this build); pass a local "
            f"snapshot laid out like the hub's, or run with --synthetic / model.prediction_model.random_init for random weights")

    # ---- frozen VAE (trainer.py:2128-2131, cast to the weight dtype :516-527)
    @property
    def vae(self):
        if self._vae is None:
            from ..models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
            root = cfg_get(self.config, "pretrained_model_name_or_path")
            local = bool(root) and os.path.isdir(os.path.join(root, "vae"))
            if not local:
                self.allow_random("VAE", os.path.join(str(root), "vae"))
            vcfg = VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1) if cfg_get(self.config, "tiny", False) else None
            self._vae = AutoencoderKL.from_pretrained(root if local else None, subfolder="vae", random_init=not local,
                                                      vae_config=vcfg, torch_dtype=self.weight_dtype, device=self.device)
        return self._vae

    # ---- frozen CLIP text encoder (trainer.py:2126-2131)
    @property
    def text_encoder(self):
        if self._text_encoder is None:
            from ..models.clip.text_encoder import CLIPTextModel, CLIPTextConfig
            root = cfg_get(self.config, "pretrained_model_name_or_path")
            local = bool(root) and os.path.isdir(os.path.join(root, "text_encoder"))
            if not local:
                self.allow_random("text encoder", os.path.join(str(root), "text_encoder"))
            tcfg = None
            if cfg_get(self.config, "tiny", False):
                tcfg = CLIPTextConfig(vocab_size=1000, hidden_size=self.unet_config.cross_attention_dim, intermediate_size=256,
                                      num_hidden_layers=2, num_attention_heads=self.unet_config.cross_attention_dim // 64)
            self._text_encoder = CLIPTextModel.from_pretrained(root if local else None, subfolder="text_encoder",
                                                               random_init=not local, text_config=tcfg,
                                                               torch_dtype=self.weight_dtype, device=self.device)
        return self._text_encoder

    @property
    def tokenizer(self):
        if self._tokenizer is None:
            from .data import load_tokenizer
            self._tokenizer = load_tokenizer(cfg_get(self.config, "pretrained_model_name_or_path"))
        return self._tokenizer

    def load_unet(self, ckpt_dir, train=False):
        """The pruned student of a trainer checkpoint directory: arch_vector.pt + unet/diffusion_pytorch_model.safetensors.
        train=True: with gradient arena and dgrad weight copies (a baseline that fine-tunes it, ESD)."""
        from ..models.unet.unet_2d_conditional import UNet2DConditionModelPruned
        arch = torch.load(os.path.join(ckpt_dir, "arch_vector.pt"), map_location="cpu")
        return UNet2DConditionModelPruned.from_pretrained(
            ckpt_dir, subfolder="unet", arch_vector=arch, unet_config=self.unet_config, torch_dtype=self.weight_dtype,
            device=self.device, train=bool(train), **unet_kwargs(self.config))

    def pipeline(self, unet, kind="pndm", scheduler=None, tokenizer=True):
        """StableDiffusionPruningPipeline over `unet` and the snapshot's VAE / text encoder, with `scheduler` or
        load_scheduler(kind).  tokenizer=False: no string prompts, so no tokenizer directory is needed."""
        from ..pipelines.pruning_pipelines import StableDiffusionPruningPipeline
        return StableDiffusionPruningPipeline(self.vae, self.text_encoder, unet, scheduler or load_scheduler(self.config, kind),
                                              self.tokenizer if tokenizer else None)
