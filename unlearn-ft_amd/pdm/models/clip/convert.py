"""CLIP checkpoints for the CLIP score, host side only (no device code): where a model name points, how an OpenAI CLIP `.pt`
(TorchScript archive or pickled state dict, as the `clip` package keeps them) maps onto transformers' CLIPModel key names,
and the text / vision configs, read from a transformers `config.json` or inferred from the tensor shapes."""
import json
import os

import torch

# the `clip` package's download names (clip/clip.py _MODELS): it keeps them as ~/.cache/clip/<basename of the URL>
OPENAI_FILES = {"ViT-B/32": "ViT-B-32.pt", "ViT-B/16": "ViT-B-16.pt", "ViT-L/14": "ViT-L-14.pt",
                "ViT-L/14@336px": "ViT-L-14-336px.pt"}
OPENAI_RESNETS = ("RN50", "RN101", "RN50x4", "RN50x16", "RN50x64")

# transformers' CLIPTextConfig / CLIPVisionConfig defaults (ViT-B/32), for config.json files that omit a field
TEXT_DEFAULTS = dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                     max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act="quick_gelu")
VISION_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=224,
                       patch_size=32, layer_norm_eps=1e-5, hidden_act="quick_gelu")


def model_tag(clip_model):
    """Directory tag of the feature files: `ViT-B/32` -> `ViT-B-32`; a path -> its basename without extension."""
    if clip_model in OPENAI_FILES or clip_model in OPENAI_RESNETS:
        return clip_model.replace("/", "-")
    base = os.path.basename(os.path.normpath(clip_model))
    return os.path.splitext(base)[0]


def resolve(clip_model):
    """A local `.pt` file or transformers directory; an OpenAI model name resolves to ~/.cache/clip/<file>."""
    if clip_model in OPENAI_RESNETS:
        raise NotImplementedError(f"{clip_model}: ResNet CLIP image towers are not implemented (ViT models only)")
    if os.path.exists(clip_model):
        return clip_model
    if clip_model in OPENAI_FILES:
        path = os.path.join(os.path.expanduser("~"), ".cache", "clip", OPENAI_FILES[clip_model])
        if os.path.exists(path):
            return path
        raise FileNotFoundError(f"{clip_model!r}: {path} does not exist and downloads are not available to this build; "
                                f"place the clip package's checkpoint there or pass a local path")
    raise FileNotFoundError(f"{clip_model!r} is not a local file or directory and hub downloads are not available to this "
                            f"build; pass a local transformers directory or an OpenAI CLIP .pt file")


def load_openai_state_dict(path):
    """OpenAI CLIP `.pt`: a TorchScript archive (what the clip package downloads) or a pickled state dict."""
    try:
        return {k: v for k, v in torch.jit.load(path, map_location="cpu").state_dict().items()}
    except Exception:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(sd, dict):
            raise ValueError(f"{path}: neither a TorchScript archive nor a pickled state dict")
        return dict(sd.get("state_dict", sd))


def _layers(sd, prefix):
    return len({k[len(prefix):].split(".")[0] for k in sd if k.startswith(prefix)})


def openai_configs(sd):
    """(text config dict, vision config dict, projection_dim) inferred from an OpenAI state dict's shapes."""
    if "visual.conv1.weight" not in sd:
        if any(k.startswith("visual.layer1.") for k in sd):
            raise NotImplementedError("ResNet CLIP image towers are not implemented (ViT models only)")
        raise ValueError("not an OpenAI CLIP state dict (no visual.conv1.weight)")
    w = sd["visual.conv1.weight"]
    width, patch = int(w.shape[0]), int(w.shape[-1])
    grid = round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    vision = dict(hidden_size=width, patch_size=patch, image_size=patch * grid,
                  num_hidden_layers=_layers(sd, "visual.transformer.resblocks."), num_attention_heads=width // 64,
                  intermediate_size=int(sd["visual.transformer.resblocks.0.mlp.c_fc.weight"].shape[0]),
                  layer_norm_eps=1e-5, hidden_act="quick_gelu")
    tw = int(sd["ln_final.weight"].shape[0])
    text = dict(vocab_size=int(sd["token_embedding.weight"].shape[0]), hidden_size=tw,
                intermediate_size=int(sd["transformer.resblocks.0.mlp.c_fc.weight"].shape[0]),
                num_hidden_layers=_layers(sd, "transformer.resblocks."), num_attention_heads=tw // 64,
                max_position_embeddings=int(sd["positional_embedding"].shape[0]), layer_norm_eps=1e-5,
                hidden_act="quick_gelu")
    return text, vision, int(sd["text_projection"].shape[1])


def _block(out, src, dst, sd):
    ipw, ipb = sd[src + "attn.in_proj_weight"], sd[src + "attn.in_proj_bias"]
    E = ipw.shape[1]
    for i, n in enumerate("qkv"):
        out[f"{dst}self_attn.{n}_proj.weight"] = ipw[i * E:(i + 1) * E]
        out[f"{dst}self_attn.{n}_proj.bias"] = ipb[i * E:(i + 1) * E]
    for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                 ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
        out[f"{dst}{b}.weight"], out[f"{dst}{b}.bias"] = sd[f"{src}{a}.weight"], sd[f"{src}{a}.bias"]


def openai_to_hf(sd):
    """OpenAI CLIP key names -> transformers CLIPModel key names (in_proj split into q / k / v; `visual.proj` and
    `text_projection` are x @ P, transformers' projections are Linear weights: transposed)."""
    text, vision, _ = openai_configs(sd)
    out = {"vision_model.embeddings.class_embedding": sd["visual.class_embedding"],
           "vision_model.embeddings.patch_embedding.weight": sd["visual.conv1.weight"],
           "vision_model.embeddings.position_embedding.weight": sd["visual.positional_embedding"],
           "vision_model.pre_layrnorm.weight": sd["visual.ln_pre.weight"], "vision_model.pre_layrnorm.bias": sd["visual.ln_pre.bias"],
           "vision_model.post_layernorm.weight": sd["visual.ln_post.weight"],
           "vision_model.post_layernorm.bias": sd["visual.ln_post.bias"],
           "visual_projection.weight": sd["visual.proj"].t().contiguous(),
           "text_model.embeddings.token_embedding.weight": sd["token_embedding.weight"],
           "text_model.embeddings.position_embedding.weight": sd["positional_embedding"],
           "text_model.final_layer_norm.weight": sd["ln_final.weight"], "text_model.final_layer_norm.bias": sd["ln_final.bias"],
           "text_projection.weight": sd["text_projection"].t().contiguous(),
           "logit_scale": sd["logit_scale"]}
    for i in range(vision["num_hidden_layers"]):
        _block(out, f"visual.transformer.resblocks.{i}.", f"vision_model.encoder.layers.{i}.", sd)
    for i in range(text["num_hidden_layers"]):
        _block(out, f"transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}.", sd)
    return out


def read_hf_dir(path):
    """(text config, vision config, projection_dim, state dict) of a local transformers CLIPModel directory."""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    text = {k: (cfg.get("text_config") or {}).get(k, v) for k, v in TEXT_DEFAULTS.items()}
    vision = {k: (cfg.get("vision_config") or {}).get(k, v) for k, v in VISION_DEFAULTS.items()}
    f = os.path.join(path, "model.safetensors")
    if os.path.exists(f):
        from safetensors.torch import load_file
        sd = load_file(f)
    else:
        sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    return text, vision, int(cfg.get("projection_dim", 512)), sd


def load_checkpoint(clip_model):
    """(text config, vision config, projection_dim, transformers-named state dict) of a model name or local path."""
    path = resolve(clip_model)
    if os.path.isdir(path):
        return read_hf_dir(path)
    sd = load_openai_state_dict(path)
    text, vision, proj = openai_configs(sd)
    return text, vision, proj, openai_to_hf(sd)
