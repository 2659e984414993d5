"""`CLIPTextModel` on libpdmk - the text conditioning path.

The reference encodes captions inside its dataset transform, per sample and twice (caption + empty prompt), with
transformers' CLIPTextModel on the training device (pdm/utils/data_utils.py:155-191, 247-276; model loaded at
pdm/training/trainer.py:2126-2131):   prompt_embeds = text_encoder(text_input_ids)[0]   # [B, 77, 1024]
Same call surface here (`from_pretrained(path, subfolder="text_encoder")`, `model(input_ids)[0]` /
`.last_hidden_state`, transformers state-dict key names with or without the `text_model.` prefix); arithmetic in
libpdmk: fused token+position gather, LayerNorm, one fused q|k|v projection, causal flash attention (head dim 64, the
U-Net's kernel with a mask), erf-GELU MLP, residuals in the GEMM epilogues.  Inference only (frozen); no CPU path.
Tokenisation stays on the host (transformers' CLIPTokenizer needs its vocabulary files): callers pass token ids.
"""
import os
from dataclasses import dataclass
from types import SimpleNamespace

import torch

from ... import _pdmk as k
from ...utils.replay import ReplayCache
from ..ops import Act, Ops, _ld
from ..unet.params import ParamStore, _lin, assign_offsets, lin_pair, load_local_or_random, norm_pair


@dataclass(frozen=True)
class CLIPTextConfig:
    vocab_size: int = 49408
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 23
    num_attention_heads: int = 16
    max_position_embeddings: int = 77
    layer_norm_eps: float = 1e-5
    hidden_act: str = "gelu"          # "gelu" (SD-2.1's OpenCLIP encoder) or "quick_gelu" (OpenAI CLIP)

    @staticmethod
    def sd21():
        return CLIPTextConfig()


def encoder_layer_entries(p, E, F):
    """One encoder layer of either tower (q|k|v fused row-wise): the parameters `encoder_layer` reads."""
    return (norm_pair(p + ".layer_norm1", E) +
            lin_pair(p + ".self_attn.qkv_proj", [(f"{p}.self_attn.{n}_proj", E) for n in ("q", "k", "v")], E) +
            lin_pair(p + ".self_attn.out_proj", [(p + ".self_attn.out_proj", E)], E) +
            norm_pair(p + ".layer_norm2", E) +
            lin_pair(p + ".mlp.fc1", [(p + ".mlp.fc1", F)], E) +
            lin_pair(p + ".mlp.fc2", [(p + ".mlp.fc2", E)], F))


def build_entries(cfg: CLIPTextConfig, projection_dim=0):
    E = cfg.hidden_size
    out = [_lin("embeddings.token_embedding", [("embeddings.token_embedding.weight", cfg.vocab_size)], E),
           _lin("embeddings.position_embedding", [("embeddings.position_embedding.weight", cfg.max_position_embeddings)], E)]
    for i in range(cfg.num_hidden_layers):
        out += encoder_layer_entries(f"encoder.layers.{i}", E, cfg.intermediate_size)
    out += norm_pair("final_layer_norm", E)
    if projection_dim:                  # CLIPModel's text_projection (no bias)
        out.append(_lin("text_projection", [("text_projection.weight", projection_dim)], E))
    return assign_offsets(out)


def encoder_layer(o, x, p, B, H, N, act, lse, causal):
    """One pre-LN transformer layer of CLIP's text (causal) / vision encoders on the 2-D activation x [B*N, E]; o: the Ops over
    the tower's parameters, p: the layer's key prefix, lse: the [B, H, N] fp32 buffer the attention kernel writes its row
    statistics to (one per forward pass, handed to every layer: inference never reads it back)."""
    E = x.t.shape[1]
    h = o.layernorm(x, p + ".layer_norm1")
    qkv = o.linear(h, p + ".self_attn.qkv_proj", bias=p + ".self_attn.qkv_proj.bias").t
    att = torch.empty((B * N, E), device=o.dev, dtype=o.dtype)
    q, kk, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:3 * E]
    st = (N * _ld(qkv), _ld(qkv))
    if causal:
        k.attn_fwd_causal(q, kk, v, att, lse, B, H, N, st, st, st, (N * E, E), 64 ** -0.5)
    else:
        k.attn_fwd(q, kk, v, att, lse, B, H, N, N, st, st, st, (N * E, E), 64 ** -0.5)
    x = o.linear(Act(att), p + ".self_attn.out_proj", bias=p + ".self_attn.out_proj.bias", residual=x)
    h = o.layernorm(x, p + ".layer_norm2")
    f = o.linear(h, p + ".mlp.fc1", bias=p + ".mlp.fc1.bias").t
    a = torch.empty_like(f)
    (k.quick_gelu_fwd if act == "quick_gelu" else k.gelu_fwd)(f, a)
    return o.linear(Act(a), p + ".mlp.fc2", bias=p + ".mlp.fc2.bias", residual=x)


class _Output(tuple):
    """`model(ids)[0]` and `model(ids).last_hidden_state`, like transformers' BaseModelOutputWithPooling."""

    @property
    def last_hidden_state(self):
        return self[0]


class CLIPTextModel:
    def __init__(self, cfg: CLIPTextConfig = None, device=None, dtype=torch.bfloat16, seed=0, init=True, projection_dim=0):
        if not torch.cuda.is_available():
            raise RuntimeError("CLIPTextModel (MI355X engine) needs a GPU; there is no CPU fallback")
        self.cfg = cfg or CLIPTextConfig.sd21()
        assert self.cfg.hidden_size // self.cfg.num_attention_heads == 64, "attention kernels are specialised for head dim 64"
        assert self.cfg.hidden_size % 32 == 0 and self.cfg.intermediate_size % 32 == 0
        if self.cfg.hidden_act not in ("gelu", "quick_gelu"):
            raise NotImplementedError(f"hidden_act {self.cfg.hidden_act!r}")
        self.device = torch.device(device or "cuda:0")
        self.dtype = dtype
        self.store = ParamStore(build_entries(self.cfg, projection_dim), self.device, dtype, train=False)
        self.ops = Ops(self.store, dtype)
        self.config = SimpleNamespace(**self.cfg.__dict__)
        # ~10 launches per layer on 77-token inputs are launch-bound from Python (3.2 ms eager for 23 layers): each
        # (B, T) shape is captured once as a hipGraph and replayed on a static id buffer
        self.use_graph = os.environ.get("PDMK_CLIP_GRAPH", "1") != "0"
        self._graphs = ReplayCache(self.device)
        if init:
            self.store.init_random(seed)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, subfolder=None, revision=None, random_init=False,
                        text_config=None, torch_dtype=torch.bfloat16, device=None, seed=0, **unused):
        return load_local_or_random(lambda init: cls(text_config, device, torch_dtype, seed=seed, init=init),
                                    pretrained_model_name_or_path, subfolder, random_init,
                                    ("model.safetensors", "pytorch_model.bin"))

    def load_state_dict(self, sd, strict=True):
        own = {}
        for key, v in sd.items():
            key = key[len("text_model."):] if key.startswith("text_model.") else key
            if key.endswith("position_ids"):
                continue
            own[key] = v
        self.store.load_state_dict(own, strict=strict)

    def state_dict(self, prefix="text_model."):
        return {prefix + n: t for n, t in self.store.state_dict().items()}

    def requires_grad_(self, flag=False):
        return self

    def to(self, *a, **kw):
        return self

    def eval(self):
        return self

    @property
    def dtype_(self):
        return self.dtype

    # ------------------------------------------------------------------ forward
    def encode_2d(self, input_ids, final_norm=True):
        """ids [B, T] (T <= 77) -> last hidden state as a 2-D [B*T, hidden] matrix in the compute dtype (final_norm=False:
        before final_layer_norm, for callers that normalise only the rows they pool)."""
        cfg, o, P = self.cfg, self.ops, self.store
        B, T = input_ids.shape
        assert T <= cfg.max_position_embeddings
        E, H = cfg.hidden_size, cfg.num_attention_heads
        ids = input_ids.to(self.device, torch.int64).contiguous()
        x = torch.empty((B * T, E), device=self.device, dtype=self.dtype)
        k.embed_tokens(ids, P.wv("embeddings.token_embedding.weight"), P.wv("embeddings.position_embedding.weight"), x,
                       B * T, T, E, cfg.vocab_size, E, E, E)
        x = Act(x, rg=False)
        lse = torch.empty((B, H, T), device=self.device, dtype=torch.float32)
        for i in range(cfg.num_hidden_layers):
            x = encoder_layer(o, x, f"encoder.layers.{i}", B, H, T, cfg.hidden_act, lse, causal=True)
        return o.layernorm(x, "final_layer_norm").t if final_norm else x.t

    def __call__(self, input_ids, output_hidden_states=False, **unused):
        B, T = input_ids.shape
        capturing = torch.cuda.is_current_stream_capturing()
        if self.use_graph and not capturing:
            y = self._graphs.run((B, T), self.encode_2d, input_ids, torch.int64)
        else:
            y = self.encode_2d(input_ids)
        return _Output((y.view(B, T, self.cfg.hidden_size),))


def encode_prompt(tokenizer, text_encoder, prompt, max_sequence_length=77, device=None, text_input_ids=None, pooled=False):
    """pdm/utils/data_utils.py:155-191 with the same signature: tokenise on the host when a tokenizer is given, else take
    `text_input_ids`; returns prompt_embeds [B, T, hidden] in the encoder's dtype."""
    if pooled:
        raise NotImplementedError("pooled CLIP output is only used by the SDXL/Flux trainers (out of scope, SURVEY 2.1)")
    prompt = [prompt] if isinstance(prompt, str) else prompt
    if tokenizer is not None:
        text_input_ids = tokenizer(prompt, padding="max_length", max_length=max_sequence_length, truncation=True,
                                   return_length=False, return_overflowing_tokens=False, return_tensors="pt").input_ids
    elif text_input_ids is None:
        raise ValueError("text_input_ids must be provided when the tokenizer is not specified")
    return text_encoder(text_input_ids)[0]
