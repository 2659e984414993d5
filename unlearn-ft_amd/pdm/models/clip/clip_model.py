"""`CLIPVisionModel` and `CLIPModel` on libpdmk - the CLIP score's encoders (pdm/utils/clip_utils.py).

The reference scores with OpenAI CLIP (`clip.load("ViT-B/32")`, pdm/utils/clip_utils.py): image features
`encode_image(preprocess(img))`, text features `encode_text(clip.tokenize(caption))`.  Same arithmetic here as transformers'
CLIPModel computes it: the ViT tower is patch im2col -> one GEMM (the stride-p conv, no bias) -> [CLS | patches] + position
-> pre_layrnorm -> pre-LN encoder layers (the text encoder's layer code without the mask: fused q|k|v GEMM, flash
attention, quick-GELU MLP, residuals in the epilogues) -> CLS row -> post_layernorm -> visual_projection.  The text tower is
CLIPTextModel up to its last layer, then the row at the first argmax of the ids (EOT), final_layer_norm on those rows only,
text_projection.  Features come out in fp32.  Any ViT CLIP whose heads are 64 wide (B/32, B/16, L/14); inference only.
Each (tower, batch shape) is captured once as a single-stream hipGraph and replayed (PDMK_CLIP_GRAPH=0: eager).
"""
import math
import os
from dataclasses import dataclass

import torch

from ... import _pdmk as k
from ...utils.replay import ReplayCache
from ..ops import Act, Ops
from ..unet.params import ParamStore, _lin, _vec, assign_offsets, norm_pair
from . import convert
from .text_encoder import CLIPTextConfig, CLIPTextModel, encoder_layer, encoder_layer_entries


@dataclass(frozen=True)
class CLIPVisionConfig:
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    image_size: int = 224
    patch_size: int = 32
    layer_norm_eps: float = 1e-5
    hidden_act: str = "quick_gelu"

    @property
    def num_positions(self):
        return (self.image_size // self.patch_size) ** 2 + 1


def build_vision_entries(cfg: CLIPVisionConfig, projection_dim=0):
    E, p = cfg.hidden_size, cfg.patch_size
    out = [_vec("embeddings.class_embedding", [("embeddings.class_embedding", E)]),
           _lin("embeddings.patch_embedding", [("embeddings.patch_embedding.weight", E)], 3 * p * p),
           _lin("embeddings.position_embedding", [("embeddings.position_embedding.weight", cfg.num_positions)], E)]
    out += norm_pair("pre_layrnorm", E)
    for i in range(cfg.num_hidden_layers):
        out += encoder_layer_entries(f"encoder.layers.{i}", E, cfg.intermediate_size)
    out += norm_pair("post_layernorm", E)
    if projection_dim:
        out.append(_lin("visual_projection", [("visual_projection.weight", projection_dim)], E))
    return assign_offsets(out)


class CLIPVisionModel:
    """transformers' CLIPVisionModel(+ visual_projection when projection_dim > 0) on libpdmk; state-dict keys with or
    without the `vision_model.` prefix."""

    def __init__(self, cfg: CLIPVisionConfig = None, device=None, dtype=torch.float32, seed=0, init=True, projection_dim=0):
        if not torch.cuda.is_available():
            raise RuntimeError("CLIPVisionModel (MI355X engine) needs a GPU; there is no CPU fallback")
        self.cfg = cfg or CLIPVisionConfig()
        c = self.cfg
        assert c.hidden_size // c.num_attention_heads == 64, "attention kernels are specialised for head dim 64"
        assert c.hidden_size % 32 == 0 and c.intermediate_size % 32 == 0 and c.image_size % c.patch_size == 0
        if c.hidden_act not in ("gelu", "quick_gelu"):
            raise NotImplementedError(f"hidden_act {c.hidden_act!r}")
        self.device, self.dtype, self.projection_dim = torch.device(device or "cuda:0"), dtype, projection_dim
        self.store = ParamStore(build_vision_entries(c, projection_dim), self.device, dtype, train=False)
        self.ops = Ops(self.store, dtype)
        if init:
            self.store.init_random(seed)

    def load_state_dict(self, sd, strict=True):
        own = {}
        for key, v in sd.items():
            key = key[len("vision_model."):] if key.startswith("vision_model.") else key
            if not key.endswith("position_ids"):
                own[key] = v
        self.store.load_state_dict(own, strict=strict)

    def pooled(self, pixel_values):
        """pixel_values fp32 [B, 3, S, S] -> post_layernorm(CLS row) [B, E] in the compute dtype (2-D Act)."""
        cfg, o, P, dev = self.cfg, self.ops, self.store, self.device
        B = pixel_values.shape[0]
        S, p, E, H = cfg.image_size, cfg.patch_size, cfg.hidden_size, cfg.num_attention_heads
        assert tuple(pixel_values.shape[1:]) == (3, S, S), f"pixel_values {tuple(pixel_values.shape)}, expected [B, 3, {S}, {S}]"
        G2, N = (S // p) ** 2, cfg.num_positions
        cols = torch.empty((B * G2, P.by_key["embeddings.patch_embedding.weight"].shape[1]), device=dev, dtype=self.dtype)
        k.patch_im2col(pixel_values.to(dev, torch.float32).contiguous(), cols, B, S, p)
        pe = o.linear(Act(cols, rg=False), "embeddings.patch_embedding").t
        x = torch.empty((B * N, E), device=dev, dtype=self.dtype)
        k.vit_tokens(pe, P.wv("embeddings.class_embedding"), P.wv("embeddings.position_embedding.weight"), E, x, B, G2, E)
        x = o.layernorm(Act(x, rg=False), "pre_layrnorm")
        lse = torch.empty((B, H, N), device=dev, dtype=torch.float32)
        for i in range(cfg.num_hidden_layers):
            x = encoder_layer(o, x, f"encoder.layers.{i}", B, H, N, cfg.hidden_act, lse, causal=False)
        cls = torch.empty((B, E), device=dev, dtype=self.dtype)
        k.gather_rows(x.t, None, N, cls, B, E)
        return o.layernorm(Act(cls, rg=False), "post_layernorm")

    def features(self, pixel_values):
        """visual_projection(pooled) [B, projection_dim] fp32."""
        y = self.ops.linear(self.pooled(pixel_values), "visual_projection", out_f32=True).t
        return y[:, :self.projection_dim]


class CLIPModel:
    """encode_image(pixel_values [B, 3, S, S]) / encode_text(input_ids [B, T]) -> [B, projection_dim] fp32 features (not
    normalised), logit_scale (fp32 scalar on the host), as OpenAI CLIP and transformers' CLIPModel expose them."""

    def __init__(self, text_cfg: CLIPTextConfig, vision_cfg: CLIPVisionConfig, projection_dim=512, device=None,
                 dtype=torch.float32, seed=0, init=True):
        self.device, self.dtype, self.projection_dim = torch.device(device or "cuda:0"), dtype, int(projection_dim)
        self.text = CLIPTextModel(text_cfg, self.device, dtype, seed=seed, init=init, projection_dim=self.projection_dim)
        self.text.use_graph = False
        self.vision = CLIPVisionModel(vision_cfg, self.device, dtype, seed=seed + 1, init=init,
                                      projection_dim=self.projection_dim)
        self.logit_scale = torch.tensor(math.log(1 / 0.07), dtype=torch.float32)
        self.use_graph = os.environ.get("PDMK_CLIP_GRAPH", "1") != "0"
        self._graphs = ReplayCache(self.device)

    @property
    def image_size(self):
        return self.vision.cfg.image_size

    @property
    def context_length(self):
        return self.text.cfg.max_position_embeddings

    @classmethod
    def from_configs(cls, text, vision, projection_dim, **kw):
        return cls(CLIPTextConfig(**text), CLIPVisionConfig(**vision), projection_dim, **kw)

    @classmethod
    def from_pretrained(cls, clip_model="ViT-B/32", dtype=torch.float32, device=None):
        """A local transformers CLIPModel directory, an OpenAI CLIP `.pt`, or an OpenAI model name (~/.cache/clip)."""
        text, vision, proj, sd = convert.load_checkpoint(clip_model)
        model = cls.from_configs(text, vision, proj, device=device, dtype=dtype, init=False)
        model.load_state_dict(sd)
        return model

    def load_state_dict(self, sd, strict=True):
        """transformers CLIPModel key names (text_model.*, vision_model.*, visual_projection.weight, text_projection.weight,
        logit_scale)."""
        text = {n: v for n, v in sd.items() if n.startswith("text_model.") or n == "text_projection.weight"}
        vision = {n: v for n, v in sd.items() if n.startswith("vision_model.") or n == "visual_projection.weight"}
        if "logit_scale" not in sd:
            raise KeyError("missing key logit_scale")
        if strict:
            extra = set(sd) - set(text) - set(vision) - {"logit_scale"}
            if extra:
                raise KeyError(f"unexpected keys in state dict: {sorted(extra)[:5]} ...")
        self.text.load_state_dict(text, strict=strict)
        self.vision.load_state_dict(vision, strict=strict)
        self.logit_scale = sd["logit_scale"].detach().to(torch.float32).cpu().reshape(())
        self._graphs.clear()

    # ------------------------------------------------------------------ forward
    def _image(self, pixel_values):
        return self.vision.features(pixel_values)

    def _text(self, input_ids):
        t, cfg = self.text, self.text.cfg
        B, T = input_ids.shape
        E = cfg.hidden_size
        ids = input_ids.to(self.device, torch.int64).contiguous()
        x = t.encode_2d(ids, final_norm=False)
        eot = torch.empty((B, E), device=self.device, dtype=self.dtype)
        k.gather_rows(x, ids, T, eot, B, E)
        h = t.ops.layernorm(Act(eot, rg=False), "final_layer_norm")
        return t.ops.linear(h, "text_projection", out_f32=True).t[:, :self.projection_dim]

    def _run(self, kind, fn, inp):
        if not self.use_graph or torch.cuda.is_current_stream_capturing():
            return fn(inp).clone()
        return self._graphs.run((kind, tuple(inp.shape)), fn, inp)

    def encode_image(self, pixel_values):
        return self._run("image", self._image, pixel_values.to(self.device, torch.float32))

    def encode_text(self, input_ids):
        return self._run("text", self._text, input_ids.to(self.device, torch.int64))
