"""`StableDiffusionPruningPipeline.generate_samples` on libpdmk - image logging / FID sampling.

Mirror of pdm/pipelines/pruning_pipelines.py:867-1010 as scripts/metrics/generate_fid_images.py:113-153 drives it:
PNDM (PLMS, skip_prk_steps) scheduler, classifier-free guidance on a doubled batch, `vae.decode(latents /
scaling_factor)`, `image / 2 + 0.5` clamped to [0, 1].  Models are this package's `UNet2DConditionModelPruned`,
`AutoencoderKL`, `CLIPTextModel`; the scheduler's per-step latent arithmetic runs in `pdmk_axpby` (fp32), its scalar
coefficients on the host in float64 like diffusers.  Prompts come as token ids, embeddings or - with a tokenizer - strings.
The safety checker of the diffusers base class is not reproduced (the reference's FID script keeps every image).
Scheduler parity is "unpinned" (diffusers absent, no vendored twin): see oracle/pdm_ref/sampler.py.

The denoising loop runs as replays of a captured graph (`_CapturedLoop`) when it can: one U-Net forward on static buffers
followed by pdmk_plms_step, which does the guidance, the PLMS update and the next U-Net input in one launch, advances a
device-side step counter and refreshes the U-Net's timestep buffer from a step table - so one capture serves every step.
It is bit-identical to the eager loop (the kernel repeats pdmk_axpby's fp32 arithmetic operation by operation; DESIGN.md
9.1).  `callback=`, block hooks, an `ffn_observer` on the U-Net's engine or PDMK_SAMPLER_GRAPH=0 select the eager loop; so
does a DDIMScheduler unless the caller passes graph=True (pdmk_ddim_step is then the step kernel).

Safe Latent Diffusion (`safety_concept=` and the `sld_*` keywords) adds a third row block conditioned on a safety
concept: the eager loop calls pdmk_sld_guidance before scheduler.step, the captured loop's step kernel is pdmk_sld_plms_step /
pdmk_sld_ddim_step on 3B rows.  With SLD off nothing of it runs: the same loops, launches and bits as without the keywords.

Concept algebra (`algebra_concepts=` / `algebra_ids=` / `algebra_embeds=`) runs five row blocks - uncond, text
and three concept prompts - and projects the text score off the direction between the first two concepts: pdmk_calg_dots
leaves the two sums over the whole batch as fp64 partials, then pdmk_calg_guidance (eager) or pdmk_calg_plms_step /
pdmk_calg_ddim_step (captured, 5B rows) applies them.  Without the keyword nothing of it runs.

K-LMS (`LMSDiscreteScheduler`, what the reference's UCE evaluation scripts sample with) calls the U-Net at
fractional float32 timesteps on inputs divided by sqrt(sigma^2 + 1).  Its loop is captured by default like PNDM's, with
pdmk_lms_step / pdmk_sld_lms_step / pdmk_calg_lms_step as the step kernel (the next input's division included), one replay per step.

ConceptPrune's neuron removal (`neuron_masks=`, a utils.concept_prune.TimestepMasks) sets the ff.net.2 compute
weights to W * (1 - mask[t]) before every U-Net call: one pdmk_masked_weights launch, from the host slot in the eager loop and
from the device-side call counter as the first node of the captured graph.  The weights are restored when the call ends.
Without the keyword nothing of it runs.
"""
import ctypes
import gc
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from .. import _pdmk as k
from ..models.unet.spec import padc
from ..utils.sld import is_active as sld_is_active
from ..utils.concept_algebra import check_sampling as check_algebra


# Adams-Bashforth weights of the linear multistep update by history length, newest model output first (PLMS)
_PLMS_COEF = {2: (3 / 2, -1 / 2), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}


class _Scheduler:
    """What the schedulers share: SD-2.1's scaled_linear betas, the `config` namespace, the strict `from_config` and the
    identity `scale_model_input` (LMS overrides it).  A subclass sets the key tables and has `set_timesteps` and `step`."""
    order = 1
    init_noise_sigma = 1.0
    _FIXED = {}          # config keys whose value the class does not implement otherwise: the value it implements
    _FREE = ("num_train_timesteps", "beta_start", "beta_end", "steps_offset", "prediction_type")      # __init__'s arguments
    _IGNORED = ()        # keys read only by what _FIXED turns off, or by the other class

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 prediction_type="epsilon"):
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"{type(self).__name__}: prediction_type={prediction_type!r} is not implemented")
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).double()
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, steps_offset=steps_offset,
                                      prediction_type=prediction_type)
        self.timesteps = None

    @classmethod
    def from_config(cls, config):
        """From a diffusers scheduler_config.json dict (or its path).  Keys starting with "_" and the class's _IGNORED ones
        are skipped; a value this class does not implement (PRK steps, another beta schedule, set_alpha_to_one, clipping,
        thresholding, trailing spacing, ...) or an unknown key raises."""
        if isinstance(config, str):
            with open(config) as f:
                config = json.load(f)
        kw = {}
        for key, v in config.items():
            if key.startswith("_") or key in cls._IGNORED:
                continue
            if key in cls._FIXED:
                if v != cls._FIXED[key]:
                    raise ValueError(f"{cls.__name__}: {key}={v!r} is not implemented (only {cls._FIXED[key]!r})")
            elif key in cls._FREE:
                kw[key] = v
            else:
                raise ValueError(f"{cls.__name__}: config key {key!r} is not implemented")
        return cls(**kw)

    def _ratio(self):
        return self.config.num_train_timesteps // self.num_inference_steps

    def scale_model_input(self, sample, t=None):
        return sample


class PNDMScheduler(_Scheduler):
    """diffusers PNDMScheduler as configured by SD-2.1's scheduler_config.json (skip_prk_steps, steps_offset 1,
    set_alpha_to_one False, scaled_linear betas)."""
    _FIXED = {"beta_schedule": "scaled_linear", "skip_prk_steps": True, "set_alpha_to_one": False, "trained_betas": None,
              "clip_sample": False, "timestep_spacing": "leading"}

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.config.skip_prk_steps = True

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        base = (torch.arange(0, num_inference_steps) * self._ratio()).round().long() + self.config.steps_offset
        self.timesteps = torch.cat([base[:-1], base[-2:-1], base[-1:]]).flip(0)
        self.ets, self.counter, self.cur_sample = [], 0, None

    def step(self, model_output, timestep, sample, return_dict=True):
        """model_output / sample: contiguous fp32 device tensors of one shape; returns the previous sample (new tensor)."""
        t = int(timestep)
        ratio = self._ratio()
        prev_t = t - ratio
        if self.counter != 1:
            self.ets = self.ets[-3:] + [model_output]
        else:
            prev_t, t = t, t + ratio
        e = self.ets
        mo = model_output.clone()
        if len(e) == 1 and self.counter == 0:
            self.cur_sample = sample
        elif len(e) == 1 and self.counter == 1:
            k.axpby(e[-1], mo, 0.5, 0.5)                                   # (model_output + ets[-1]) / 2
            sample, self.cur_sample = self.cur_sample, None
        else:
            coef = _PLMS_COEF[len(e)]
            mo.copy_(e[-1])
            k.axpby(e[-2], mo, coef[1], coef[0])
            for i in range(2, len(e)):
                k.axpby(e[-1 - i], mo, coef[i], 1.0)
        self.counter += 1
        v_x, v_v, eps_scale, x_scale = self._scalars(t, prev_t)
        if self.config.prediction_type == "v_prediction":
            k.axpby(sample, mo, v_x, v_v)                                  # eps = sqrt(a) v + sqrt(1 - a) x
        prev = sample.clone()
        k.axpby(mo, prev, eps_scale, x_scale)                              # coeff * sample - (a_prev - a_t) eps / denom
        return SimpleNamespace(prev_sample=prev) if return_dict else (prev,)

    def _scalars(self, t, prev_t):
        """The step's coefficients (float64, then Python floats; fp32 where a kernel takes them): the v -> eps conversion
        (sqrt(1 - a_t), sqrt(a_t)) and prev = x_scale * sample + eps_scale * eps."""
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t, b_prev = 1 - a_t, 1 - a_prev
        coeff = float((a_prev / a_t).sqrt())
        denom = float(a_t * b_prev.sqrt() + (a_t * b_t * a_prev).sqrt())
        return float(b_t.sqrt()), float(a_t.sqrt()), -float(a_prev - a_t) / denom, coeff

    def plms_rows(self):
        """The schedule of set_timesteps() as pdmk_plms_row entries: what step() does at each index, its history (`ets`,
        at most 4 entries) kept in 4 ring slots.  The scalars are step()'s own (_scalars)."""
        ratio = self._ratio()
        rows, appended = [], 0                        # appended: entries ever added to ets (step() skips counter 1)
        for i, t in enumerate(self.timesteps.tolist()):
            r = k.PlmsRow(t=int(t), vpred=int(self.config.prediction_type == "v_prediction"))
            prev_t = t - ratio
            if i == 1:
                prev_t, t = t, t + ratio
                r.mode, r.wslot, r.nterms = 1, -1, 1
                r.rslot[0] = (appended - 1) % 4
                r.coef[0] = r.coef[1] = 0.5
            else:
                r.wslot = appended % 4
                appended += 1
                r.nterms = min(appended, 4)
                r.mode = 0 if i == 0 else 2
                for j in range(3):
                    r.rslot[j] = (appended - 2 - j) % 4
                if r.mode == 2:
                    for j, c in enumerate(_PLMS_COEF[r.nterms]):
                        r.coef[j] = c
            r.v_x, r.v_v, r.eps_scale, r.x_scale = self._scalars(t, prev_t)
            rows.append(r)
        return rows


class DDIMScheduler(_Scheduler):
    """diffusers DDIMScheduler with eta = 0 (deterministic, one U-Net call per step - what ConceptPrune's per-timestep
    accumulators count on) as SD-2.1's DDIM scheduler_config.json sets it, as far as that file can be recalled here:
    scaled_linear betas 0.00085 ... 0.012, steps_offset 1, clip_sample false, set_alpha_to_one false, leading timestep spacing.
    Unpinned like PNDMScheduler above (diffusers absent, no vendored twin).  `from_config` is as strict as PNDM's.

    With a_t = alphas_cumprod[t], b_t = 1 - a_t and a_p / b_p those of the previous timestep t - T / N (below 0: alphas_cumprod[0])
        epsilon:       prev = sqrt(a_p / a_t) x + (sqrt(b_p) - sqrt(a_p b_t / a_t)) e
        v_prediction:  prev = (sqrt(a_p a_t) + sqrt(b_p b_t)) x + (sqrt(b_p a_t) - sqrt(a_p b_t)) v
    (x0 and eps substituted into sqrt(a_p) x0 + sqrt(b_p) eps): linear in (sample, model_output), so the coefficients are
    formed in float64 on the host and the step is one pdmk_axpby launch."""
    _FIXED = {"beta_schedule": "scaled_linear", "set_alpha_to_one": False, "trained_betas": None, "clip_sample": False,
              "timestep_spacing": "leading", "thresholding": False, "rescale_betas_zero_snr": False}
    # SD-2.1's file carries PNDM's skip_prk_steps beside DDIM's class name
    _IGNORED = ("clip_sample_range", "dynamic_thresholding_ratio", "sample_max_value", "skip_prk_steps")

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        self.timesteps = ((torch.arange(0, num_inference_steps) * self._ratio()).round().long() + self.config.steps_offset).flip(0)

    def coefficients(self, t):
        """(c_x, c_m) with prev = c_x * sample + c_m * model_output, float64 arithmetic, Python floats."""
        prev_t = t - self._ratio()
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t, b_p = 1 - a_t, 1 - a_p
        if self.config.prediction_type == "v_prediction":
            return float((a_p * a_t).sqrt() + (b_p * b_t).sqrt()), float((b_p * a_t).sqrt() - (a_p * b_t).sqrt())
        return float((a_p / a_t).sqrt()), float(b_p.sqrt() - (a_p * b_t / a_t).sqrt())

    def step(self, model_output, timestep, sample, return_dict=True):
        """model_output / sample: contiguous fp32 device tensors of one shape; returns the previous sample (new tensor)."""
        c_x, c_m = self.coefficients(int(timestep))
        prev = sample.clone()
        k.axpby(model_output, prev, c_m, c_x)
        return SimpleNamespace(prev_sample=prev) if return_dict else (prev,)

    def ddim_rows(self):
        """The schedule of set_timesteps() as pdmk_ddim_row entries: step()'s coefficients at each timestep."""
        rows = []
        for t in self.timesteps.tolist():
            c_x, c_m = self.coefficients(int(t))
            rows.append(k.DdimRow(t=int(t), c_x=c_x, c_m=c_m))
        return rows


class LMSDiscreteScheduler(_Scheduler):
    """diffusers LMSDiscreteScheduler (K-LMS, Katherine Crowson's linear multistep sampler) as the UCE evaluation scripts
    configure it: scaled_linear betas 0.00085 ... 0.012, 1000 train steps, linspace timestep spacing, no Karras sigmas, order
    4.  A restatement from the published algorithm, unpinned like PNDMScheduler and DDIMScheduler above (diffusers absent,
    no vendored twin).  `from_config` is as strict as theirs; `steps_offset` is read by no linspace-spaced schedule.

    sigma_t = sqrt((1 - a_t) / a_t) from the fp32 alphas_cumprod.  set_timesteps(n): timesteps = linspace(0, T - 1, n) in
    fp32, reversed and kept FRACTIONAL (the U-Net is called at 988.9091); sigmas = interp(timesteps, arange(T), sigma_t), a
    0 appended, fp32.  init_noise_sigma = max sigma.  scale_model_input divides by sqrt(sigma_i^2 + 1) (one fp32 scalar, one
    fp32 division per element: pdmk_scale_div).  step i, with order_i = min(i + 1, 4):
        d_i  = model_output                                                           (epsilon)
        d_i  = sigma / (sigma^2 + 1) sample + 1 / sqrt(sigma^2 + 1) model_output      (v_prediction)
        c_j  = integral over [sigma_i, sigma_{i+1}] of prod_{k != j, k < order_i} (tau - sigma_{i-k}) / (sigma_{i-j} - sigma_{i-k})
        prev = sample + sum_j c_j d_{i-j}
    The coefficients are float64 host scalars and every latent operation is one pdmk_axpby, the newest derivative first.
    Two deviations from diffusers: c_j is the exact integral of the polynomial (degree <= 3; diffusers calls
    scipy.integrate.quad with epsrel 1e-4), and the derivative is formed with the fused coefficients above instead of
    diffusers' fp32 chain (sample - pred_original_sample) / sigma."""
    _FIXED = {"beta_schedule": "scaled_linear", "trained_betas": None, "use_karras_sigmas": False,
              "timestep_spacing": "linspace"}
    _IGNORED = ("steps_offset",)
    ORDER = 4            # step()'s default, the 4-slot history of pdmk_lms_step

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        acp = self.alphas_cumprod.float()                                  # (the fp32 cumprod itself)
        self.sigmas_all = ((1 - acp) / acp).sqrt().numpy()
        self.sigmas, self.derivatives = None, []

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        T = self.config.num_train_timesteps
        timesteps = np.linspace(0, T - 1, num_inference_steps, dtype=np.float32)[::-1].copy()
        sigmas = np.interp(timesteps, np.arange(0, T), self.sigmas_all)
        self.sigmas = np.concatenate([sigmas, [0.0]]).astype(np.float32)
        self.timesteps = torch.from_numpy(timesteps)
        self.init_noise_sigma = float(self.sigmas.max())
        self.derivatives = []
        self._index = {float(t): i for i, t in enumerate(timesteps)}

    def _in_div(self, i):
        """sqrt(sigma_i^2 + 1), every operation in fp32 (a Python float holding an fp32 value)."""
        s = self.sigmas[i]
        return float(np.sqrt(s * s + np.float32(1)))

    def scale_model_input(self, sample, t=None):
        """sample (contiguous fp32 device tensor) / sqrt(sigma^2 + 1) at the step index of timestep t; a new tensor."""
        out = torch.empty_like(sample)
        k.scale_div(sample, out, self._in_div(self._index[float(t)]))
        return out

    def lms_coefficients(self, i, order):
        """c_0 .. c_{order-1} of step i (float64): the Lagrange basis polynomials through sigma_i, sigma_{i-1}, ... integrated
        exactly over [sigma_i, sigma_{i+1}], in the variable u = tau - sigma_i (roots and bounds of the size of a step)."""
        s = self.sigmas.astype(np.float64)
        h = s[i + 1] - s[i]
        out = []
        for j in range(order):
            roots = [s[i - m] - s[i] for m in range(order) if m != j]
            denom = 1.0
            for m in range(order):
                if m != j:
                    denom *= s[i - j] - s[i - m]
            integral = np.polynomial.polynomial.polyint(np.polynomial.polynomial.polyfromroots(roots) if roots else [1.0])
            out.append(float(np.polynomial.polynomial.polyval(h, integral) / denom))
        return out

    def derivative_coefficients(self, i):
        """(d_x, d_m) with d = d_x * sample + d_m * model_output for v_prediction (float64); None for epsilon (d = model_output)."""
        if self.config.prediction_type != "v_prediction":
            return None
        s = float(self.sigmas[i])
        return s / (s * s + 1.0), 1.0 / (s * s + 1.0) ** 0.5

    def step(self, model_output, timestep, sample, order=ORDER, return_dict=True):
        """model_output / sample: contiguous fp32 device tensors of one shape; returns the previous sample (new tensor)."""
        i = self._index[float(timestep)]
        d, dc = model_output, self.derivative_coefficients(i)
        if dc is not None:
            d = model_output.clone()
            k.axpby(sample, d, dc[0], dc[1])
        self.derivatives = (self.derivatives + [d])[-order:]
        prev = sample.clone()
        for c, dj in zip(self.lms_coefficients(i, min(i + 1, order)), reversed(self.derivatives)):
            k.axpby(dj, prev, c, 1.0)
        return SimpleNamespace(prev_sample=prev) if return_dict else (prev,)

    def lms_rows(self):
        """The schedule of set_timesteps() as pdmk_lms_row entries: step()'s coefficients at each index, the derivative of
        step i in ring slot i % 4, and the divisor of the next call's scale_model_input (sigma 0 after the last: 1)."""
        rows = []
        for i, t in enumerate(self.timesteps.tolist()):
            r = k.LmsRow(t=t, nterms=min(i + 1, self.ORDER), wslot=i % 4, in_div=self._in_div(i + 1))
            for j in range(3):
                r.rslot[j] = (i - 1 - j) % 4
            for j, c in enumerate(self.lms_coefficients(i, r.nterms)):
                r.coef[j] = c
            dc = self.derivative_coefficients(i)
            if dc is not None:
                r.dmode, r.d_x, r.d_m = 1, dc[0], dc[1]
            rows.append(r)
        return rows


class _CapturedLoop:
    """The denoising loop of one (batch, H, W, dtype, CFG, steps, text shape, guidance) as replays of ONE single-stream
    captured graph (GraphedBilevel's docstring: graphs with parallel branches are not used): the U-Net forward over static
    buffers, then pdmk_plms_step (kind "plms"), pdmk_ddim_step (kind "ddim") or pdmk_lms_step (kind "lms"), which writes the
    next U-Net input and timesteps itself and advances the step counter.  The same graph is replayed once per U-Net call
    (N + 1 calls for N PLMS steps, N for N DDIM or LMS steps), or fewer when the caller stops early.  The graph reads the
    U-Net's weight arenas in place: it stays valid while an optimiser rewrites them."""

    def __init__(self, unet, B, h, w, cfg_on, guidance_scale, nsteps, T, ctx, kind="plms", sld=None, algebra=False, masks=None):
        dev, dt = unet.device, unet.dtype
        # utils.concept_prune.TimestepMasks: pdmk_masked_weights is the graph's FIRST node - it reads the call counter that the
        # previous replay's step kernel advanced (one stream) and sets the ff.net.2 compute weights of this call; the graph
        # holds the addresses of the masks' buffers, and the loop the object, so they live as long as it does
        self.masks = masks
        if kind not in ("plms", "ddim", "lms"):
            raise ValueError(f"_CapturedLoop: step kind {kind!r}")
        self.kind = kind
        self.Row = {"plms": k.PlmsRow, "ddim": k.DdimRow, "lms": k.LmsRow}[kind]
        self.unet, self.B, self.C, self.h, self.w, self.cfg_on, self.nsteps = unet, B, unet.cfg.in_channels, h, w, cfg_on, nsteps
        self.g = (float(1.0 - guidance_scale), float(guidance_scale))       # axpby(out[:B], out[B:], 1 - g, g)
        self.sld = sld                  # k.SldParams: the 3B form (uncond, text, safety rows; Safe Latent Diffusion guidance)
        if sld is not None and not cfg_on:
            raise ValueError("_CapturedLoop: SLD needs classifier-free guidance")
        self.algebra = bool(algebra)    # the 5B form (uncond, text, three concept rows; concept-algebra guidance)
        if self.algebra and (sld is not None or not cfg_on):
            raise ValueError("_CapturedLoop: concept algebra needs classifier-free guidance and excludes SLD")
        self.R, self.cp = (5 * B if self.algebra else 3 * B if sld is not None else 2 * B if cfg_on else B), padc(self.C)
        n = B * self.C * h * w
        self.x = torch.zeros((self.R * h * w, self.cp), device=dev, dtype=dt)
        self.t = torch.zeros(self.R, device=dev, dtype=torch.float32 if kind == "lms" else torch.int64)   # LMS: fractional
        self.ehs = torch.zeros((self.R * T, ctx), device=dev, dtype=dt)
        self.sample = torch.zeros(n, device=dev)
        if kind == "plms":
            self.cur = torch.zeros(n, device=dev)
        if kind in ("plms", "lms"):
            self.ets = torch.zeros(4, n, device=dev)    # PLMS: model outputs; LMS: derivatives
        if sld is not None:
            self.mom = torch.zeros(n, device=dev)
        if self.algebra:
            self.ws = torch.zeros(k.calg_workspace_elems(B, self.C, h * w), device=dev, dtype=torch.float64)
            self.scalars = torch.zeros(2, device=dev)
        self.state = torch.zeros(2, device=dev, dtype=torch.int32)
        self.table = torch.zeros(nsteps * ctypes.sizeof(self.Row), device=dev, dtype=torch.uint8)
        self.graph, self.keep = None, []
        self._capture()

    def _body(self):
        if self.masks is not None:
            self.masks.apply(state=self.state, repeat_first=self.kind == "plms")
        pred, _ = self.unet.forward_nhwc(self.x, self.t, self.ehs, self.R, self.h, self.w, train=False)
        if self.algebra:
            k.calg_dots(pred.t, pred.t.stride(0), self.B, self.C, self.h * self.w, self.ws)
            if self.kind == "plms":
                k.calg_plms_step(pred.t, pred.t.stride(0), self.g[1], self.ws, self.scalars, self.sample, self.cur, self.ets,
                                 self.table, self.nsteps, self.state, self.t, self.x, self.cp, self.B, self.C, self.h * self.w)
            elif self.kind == "lms":
                k.calg_lms_step(pred.t, pred.t.stride(0), self.g[1], self.ws, self.scalars, self.sample, self.ets, self.table,
                                self.nsteps, self.state, self.t, self.x, self.cp, self.B, self.C, self.h * self.w)
            else:
                k.calg_ddim_step(pred.t, pred.t.stride(0), self.g[1], self.ws, self.scalars, self.sample, self.table,
                                 self.nsteps, self.state, self.t, self.x, self.cp, self.B, self.C, self.h * self.w)
        elif self.sld is not None:
            if self.kind == "plms":
                k.sld_plms_step(pred.t, pred.t.stride(0), self.g[1], self.sld, self.mom, self.sample, self.cur, self.ets,
                                self.table, self.nsteps, self.state, self.t, self.x, self.cp, self.B, self.C, self.h * self.w)
            elif self.kind == "lms":
                k.sld_lms_step(pred.t, pred.t.stride(0), self.g[1], self.sld, self.mom, self.sample, self.ets, self.table,
                               self.nsteps, self.state, self.t, self.x, self.cp, self.B, self.C, self.h * self.w)
            else:
                k.sld_ddim_step(pred.t, pred.t.stride(0), self.g[1], self.sld, self.mom, self.sample, self.table, self.nsteps,
                                self.state, self.t, self.x, self.cp, self.B, self.C, self.h * self.w)
        elif self.kind == "plms":
            k.plms_step(pred.t, pred.t.stride(0), *self.g, self.cfg_on, self.sample, self.cur, self.ets, self.table,
                        self.nsteps, self.state, self.t, self.x, self.cp, self.B, self.C, self.h * self.w)
        elif self.kind == "lms":
            k.lms_step(pred.t, pred.t.stride(0), *self.g, self.cfg_on, self.sample, self.ets, self.table, self.nsteps,
                       self.state, self.t, self.x, self.cp, self.B, self.C, self.h * self.w)
        else:
            k.ddim_step(pred.t, pred.t.stride(0), *self.g, self.cfg_on, self.sample, self.table, self.nsteps, self.state,
                        self.t, self.x, self.cp, self.B, self.C, self.h * self.w)
        return pred

    def _capture(self):
        dev = self.x.device
        # eager warm-up of the same body (plans the GEMMs of these shapes on random operands and sizes the engine's arenas;
        # the counter is past the end, so the PLMS launch does nothing)
        gen = torch.Generator(device=dev).manual_seed(1234)
        self.x[:, :self.C].normal_(generator=gen)
        self.ehs.normal_(generator=gen)
        self.t.fill_(500)
        self.state.fill_(self.nsteps)
        cap = k.role_stream(dev, "capture")
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            self._body()
        torch.cuda.current_stream().wait_stream(cap)
        torch.cuda.synchronize()
        # like torch.cuda.graph(): collect garbage first and keep the collector off while capturing
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        self.graph = torch.cuda.CUDAGraph()
        cap.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(cap):
                self.graph.capture_begin(capture_error_mode="thread_local")
                try:
                    pred = self._body()
                finally:
                    self.graph.capture_end()
        finally:
            if gc_was_on:
                gc.enable()
        torch.cuda.current_stream().wait_stream(cap)
        torch.cuda.synchronize()
        eng = self.unet.engine          # what the graph reads or writes beyond its own pool stays allocated
        self.keep = [pred, eng.ws, eng._cs_arena]

    def run(self, latents, ehs, rows, n_calls=None, x0=None):
        """latents: fp32 [B, C, h, w] (contiguous, on the device); ehs: [R, T, ctx] text embeddings (unconditional half
        first, with SLD the safety third last, with concept algebra the three concepts last); rows: the scheduler's plms_rows() / ddim_rows() / lms_rows(); n_calls: U-Net calls to
        replay (None: all of them); x0: the first U-Net input where it is not the latents themselves (LMS: the scheduler's
        scale_model_input of them - later inputs are scaled by the step kernel).  Returns the latents after them (a new
        tensor)."""
        B, C, HW = self.B, self.C, self.h * self.w
        n_calls = self.nsteps if n_calls is None else int(n_calls)
        if len(rows) != self.nsteps or not 0 <= n_calls <= self.nsteps:
            raise ValueError(f"_CapturedLoop.run: {len(rows)} rows, {n_calls} calls for a loop of {self.nsteps}")
        self.ehs.copy_(ehs.reshape(self.ehs.shape))                       # the batch's one cast of the text embeddings
        self.table.copy_(torch.frombuffer(bytearray(bytes((self.Row * len(rows))(*rows))), dtype=torch.uint8))
        self.sample.copy_(latents.reshape(-1))
        x0 = latents if x0 is None else x0
        k.nchw_to_nhwc(x0, self.x, B, C, HW, self.cp)
        if self.cfg_on:
            k.nchw_to_nhwc(x0, self.x[B * HW:], B, C, HW, self.cp)
        if self.sld is not None:
            k.nchw_to_nhwc(x0, self.x[2 * B * HW:], B, C, HW, self.cp)
            self.mom.zero_()
        if self.algebra:
            for j in range(2, 5):
                k.nchw_to_nhwc(x0, self.x[j * B * HW:], B, C, HW, self.cp)
        self.t.fill_(rows[0].t)
        self.state.zero_()
        for _ in range(n_calls):
            self.graph.replay()
        return self.sample.view(B, C, self.h, self.w).clone()

    def close(self):
        torch.cuda.synchronize()
        self.graph, self.keep = None, []


class StableDiffusionPruningPipeline:
    GRAPH_SHAPES = 3           # captured loops kept (least recently used evicted first), like training.hip_graph_shapes

    def __init__(self, vae, text_encoder, unet, scheduler=None, tokenizer=None):
        self.vae, self.text_encoder, self.unet, self.tokenizer = vae, text_encoder, unet, tokenizer
        self.scheduler = scheduler or PNDMScheduler()
        self.vae_scale_factor = 2 ** (len(vae.cfg.block_out_channels) - 1)
        self.device = unet.device
        self._loops = {}
        self.captures = 0          # loops captured so far (tests)

    def _tokenize(self, prompt):
        if self.tokenizer is None:
            raise ValueError("string prompts need a tokenizer: pass prompt_ids / prompt_embeds, or build the pipeline with "
                             "tokenizer=")
        from ..utils.data import tokenize
        return tokenize(self.tokenizer, [prompt] if isinstance(prompt, str) else list(prompt)).to(self.device)

    def encode_prompt(self, prompt_ids=None, negative_prompt_ids=None, prompt_embeds=None, negative_prompt_embeds=None,
                      do_classifier_free_guidance=True):
        if prompt_embeds is None:
            if prompt_ids is None:
                raise ValueError("pass prompt_embeds or prompt_ids (token ids; tokenisation is host-side)")
            prompt_embeds = self.text_encoder(prompt_ids)[0]
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            if negative_prompt_ids is None:
                raise ValueError("classifier-free guidance needs negative_prompt_embeds or negative_prompt_ids "
                                 "(the tokenised empty prompt)")
            negative_prompt_embeds = self.text_encoder(negative_prompt_ids)[0]
        return prompt_embeds, negative_prompt_embeds

    def _use_graph(self, graph, callback):
        kind = type(self.scheduler)
        if graph is False or callback is not None or kind not in (PNDMScheduler, DDIMScheduler, LMSDiscreteScheduler):
            return False
        if kind is DDIMScheduler and graph is not True:      # DDIM is captured only on request
            return False
        u = self.unet
        blocks = list(getattr(u, "down_blocks", [])) + [getattr(u, "mid_block", None)] + list(getattr(u, "up_blocks", []))
        if any(getattr(b, "_hooks", None) for b in blocks):            # block hooks fire in the eager U-Net call only
            return False
        if getattr(getattr(u, "engine", None), "ffn_observer", None) is not None:     # so does a feed-forward observer
            return False
        return graph is True or os.environ.get("PDMK_SAMPLER_GRAPH", "1") != "0"

    def _loop(self, B, h, w, cfg_on, guidance_scale, nsteps, T, ctx, sld=None, algebra=False, masks=None):
        key = (B, h, w, self.unet.dtype, cfg_on, nsteps, T, ctx, float(guidance_scale), type(self.scheduler))
        if sld is not None:
            key += ("sld",) + sld.key()
        if algebra:
            key += ("algebra",)
        if masks is not None:
            key += ("masks", masks)                                   # the object: its buffers are what the graph reads
        loop = self._loops.pop(key, None)
        if loop is None:
            while len(self._loops) >= self.GRAPH_SHAPES:
                self._loops.pop(next(iter(self._loops))).close()
            loop = _CapturedLoop(self.unet, B, h, w, cfg_on, guidance_scale, nsteps, T, ctx,
                                 kind={DDIMScheduler: "ddim", LMSDiscreteScheduler: "lms"}.get(type(self.scheduler), "plms"),
                                 sld=sld, algebra=algebra, masks=masks)
            self.captures += 1
        self._loops[key] = loop                                       # most recently used last
        return loop

    @torch.no_grad()
    def generate_samples(self, prompt_ids=None, height=None, width=None, num_inference_steps=50, guidance_scale=7.5,
                         negative_prompt_ids=None, generator=None, latents=None, prompt_embeds=None,
                         negative_prompt_embeds=None, output_type="np", return_dict=True, callback=None, callback_steps=1,
                         prompt=None, negative_prompt=None, graph=None, end_iteration=None, safety_concept=None,
                         safety_concept_ids=None, safety_concept_embeds=None, sld_guidance_scale=1000.0, sld_warmup_steps=10,
                         sld_threshold=0.01, sld_momentum_scale=0.3, sld_mom_beta=0.4, algebra_concepts=None,
                         algebra_ids=None, algebra_embeds=None, neuron_masks=None):
        """prompt / negative_prompt: strings or lists of strings (needs the tokenizer; with guidance and no negative prompt
        the empty prompt).  output_type "latent", "pt", "np" (float32 NHWC in [0, 1]), "u8" (uint8 NHWC numpy, the FID
        script's `(img * 255).astype(np.uint8)`, formed on the device) or "u8_round" (the same with diffusers' numpy_to_pil
        rounding, `(img * 255).round().astype("uint8")`: the pixels of `pipeline(prompt).images`).  graph: None = the captured loop when possible
        (PDMK_SAMPLER_GRAPH=0 turns it off), False = the eager loop, True = captured whenever possible (a DDIMScheduler's loop
        is captured only with True).  end_iteration: stop after that many scheduler steps and return the latents there (ESD's
        partial sampling).
        safety_concept (a string, needs the tokenizer) / safety_concept_ids ([1, T] token ids) / safety_concept_embeds
        ([1, T, ctx]): Safe Latent Diffusion - a third U-Net branch conditioned on the concept, whose direction is subtracted
        from the guidance where the text prediction leans towards it (include/pdmk.h pdmk_sld_params; the five sld_* keywords
        default to diffusers' StableDiffusionPipelineSafe's, the Medium preset of configs/baselines/sld.yaml).  Active only
        with a concept, sld_guidance_scale > 1 and guidance_scale > 1; otherwise the keywords change nothing.  The concept is
        encoded once per call and repeated over the batch; the warm-up counts U-Net calls (PNDM's repeated call included).
        algebra_concepts (three strings, needs the tokenizer) / algebra_ids ([3, T] token ids) / algebra_embeds
        ([3, T, ctx]): concept algebra - three further U-Net branches p0, p1, p2; the text score loses its component along
        p1 - p0, measured against p2, over the whole batch (include/pdmk.h "Concept algebra").  Exactly three concepts, each
        encoded once per call and repeated over the batch; ValueError together with a safety concept or when
        guidance_scale <= 1.
        neuron_masks (utils.concept_prune.TimestepMasks of this U-Net): ConceptPrune's neuron removal - U-Net call
        t runs with the ff.net.2 weights W * (1 - mask[slot(t)]), slot(t) = t, with PNDM 0, 0, 1, 2, ...  num_inference_steps
        must be the masks' T.  DDIM (captured unless PDMK_SAMPLER_GRAPH=0, graph=False, a callback, hooks or an observer ask
        for the eager loop) and PNDM; K-LMS raises NotImplementedError, SLD or concept algebra beside the masks ValueError.
        The weights are restored when the call returns or raises.  None: nothing of it runs."""
        cfg_on = guidance_scale > 1.0
        algebra = algebra_concepts is not None or algebra_ids is not None or algebra_embeds is not None
        if algebra:
            check_algebra(guidance_scale, safety_concept is not None or safety_concept_ids is not None
                          or safety_concept_embeds is not None,
                          algebra_embeds if algebra_embeds is not None else algebra_ids if algebra_ids is not None
                          else algebra_concepts)
        has_concept = safety_concept is not None or safety_concept_ids is not None or safety_concept_embeds is not None
        sld = None
        if sld_is_active(guidance_scale, sld_guidance_scale, has_concept):
            sld = k.sld_params(sld_guidance_scale, sld_warmup_steps, sld_threshold, sld_momentum_scale, sld_mom_beta)
        if isinstance(prompt_ids, (str, list, tuple)):            # the reference's positional `prompt`
            prompt, prompt_ids = prompt_ids, None
        if prompt is not None and prompt_ids is None and prompt_embeds is None:
            prompt_ids = self._tokenize(prompt)
        if cfg_on and negative_prompt_ids is None and negative_prompt_embeds is None and (
                negative_prompt is not None or (prompt is not None and self.tokenizer is not None)):
            n = prompt_ids.shape[0] if prompt_ids is not None else prompt_embeds.shape[0]
            neg = negative_prompt if negative_prompt is not None else ""
            negative_prompt_ids = self._tokenize([neg] * n if isinstance(neg, str) else neg)
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(prompt_ids, negative_prompt_ids, prompt_embeds,
                                                                   negative_prompt_embeds, cfg_on)
        B = prompt_embeds.shape[0]
        f = self.vae_scale_factor
        if latents is not None:            # caller-provided latents fix the size (prepare_latents would reject a mismatch)
            height, width = height or latents.shape[2] * f, width or latents.shape[3] * f
        height, width = height or 64 * f, width or 64 * f     # unet.config.sample_size * vae_scale_factor at 512 px
        if height % f or width % f:
            raise ValueError(f"`height` and `width` have to be divisible by {f} but are {height} and {width}.")
        if output_type not in ("latent", "pt", "np", "u8", "u8_round"):
            raise ValueError("output_type must be 'latent', 'pt', 'np', 'u8' or 'u8_round' (PIL conversion is left to the "
                             "caller)")
        dev = self.device
        ehs = torch.cat([negative_prompt_embeds.to(dev), prompt_embeds.to(dev)]) if cfg_on else prompt_embeds.to(dev)
        if sld is not None:
            ehs = torch.cat([ehs, self._safety_embeds(safety_concept, safety_concept_ids, safety_concept_embeds, B, ehs)])
        if algebra:
            ehs = torch.cat([ehs, self._algebra_embeds(algebra_concepts, algebra_ids, algebra_embeds, B, ehs)])
        sch = self.scheduler
        sch.set_timesteps(num_inference_steps, device=dev)
        C = self.unet.cfg.in_channels
        shape = (B, C, height // f, width // f)
        if latents is None:
            latents = torch.randn(shape, device=dev, dtype=torch.float32, generator=generator)
        latents = (latents.to(dev, torch.float32) * sch.init_noise_sigma).contiguous()
        if end_iteration is not None and not 0 <= int(end_iteration) <= len(sch.timesteps):
            raise ValueError(f"end_iteration={end_iteration} outside 0 ... {len(sch.timesteps)}")
        if neuron_masks is not None:
            graph = self._check_masks(neuron_masks, num_inference_steps, graph, sld is not None or algebra)
            neuron_masks.attach()
        try:
            if self._use_graph(graph, callback):
                loop = self._loop(B, shape[2], shape[3], cfg_on, guidance_scale, len(sch.timesteps), ehs.shape[1], ehs.shape[2],
                                  sld=sld, algebra=algebra, masks=neuron_masks)
                rows = getattr(sch, loop.kind + "_rows")()
                x0 = sch.scale_model_input(latents, sch.timesteps[0].item()) if loop.kind == "lms" else None
                latents = loop.run(latents, ehs, rows, n_calls=end_iteration, x0=x0)
            else:
                latents = self._eager_loop(latents, ehs, B, shape, cfg_on, guidance_scale, callback, callback_steps,
                                           end_iteration, sld=sld, algebra=algebra, masks=neuron_masks)
        finally:
            if neuron_masks is not None:
                neuron_masks.detach()
        if output_type == "latent":
            image = latents
        else:
            image = self.vae.decode(latents / self.vae.cfg.scaling_factor, return_dict=False)[0]
            if output_type in ("u8", "u8_round"):
                b, c, hh, ww = image.shape
                u8 = torch.empty((b, hh, ww, c), device=image.device, dtype=torch.uint8)
                if output_type == "u8":
                    k.image_to_u8(image.contiguous(), u8)
                else:
                    k.image_to_u8_ex(image.contiguous(), u8, 1)
                image = u8.cpu().numpy()
            else:
                image = (image / 2 + 0.5).clamp(0, 1)                     # VaeImageProcessor.postprocess (denormalize)
                if output_type == "np":
                    image = image.permute(0, 2, 3, 1).cpu().numpy()
        return SimpleNamespace(images=image, nsfw_content_detected=None) if return_dict else (image, None)

    def _check_masks(self, masks, num_inference_steps, graph, other_guidance):
        """What neuron_masks= asks of the call; returns `graph` (a DDIM loop with masks is captured unless something asks for
        the eager one)."""
        kind = type(self.scheduler)
        if kind not in (PNDMScheduler, DDIMScheduler):                # K-LMS: nothing pins what its slots would be
            raise NotImplementedError(f"neuron_masks with {kind.__name__}: the timestep slots are defined for DDIM and PNDM only")
        if other_guidance:
            raise ValueError("neuron_masks combines with plain classifier-free guidance only, not with SLD or concept algebra")
        if getattr(masks, "unet", None) is not self.unet:
            raise ValueError("neuron_masks were built for another U-Net")
        if int(num_inference_steps) != masks.T:
            raise ValueError(f"num_inference_steps={num_inference_steps}, but the neuron masks hold {masks.T} timesteps")
        if kind is DDIMScheduler and graph is None and os.environ.get("PDMK_SAMPLER_GRAPH", "1") != "0":
            graph = True
        return graph

    def _safety_embeds(self, concept, ids, embeds, B, ehs):
        """The safety concept's text embeddings [B, T, ctx]: encoded once, repeated over the batch."""
        if embeds is None:
            if ids is None:
                ids = self._tokenize(concept if isinstance(concept, str) else list(concept))
            embeds = self.text_encoder(ids.to(self.device))[0]
        embeds = embeds.to(self.device)
        if embeds.dim() == 2:
            embeds = embeds[None]
        if embeds.shape[0] != 1 or tuple(embeds.shape[1:]) != tuple(ehs.shape[1:]):
            raise ValueError(f"safety concept embeddings {tuple(embeds.shape)}: expected one concept of shape "
                             f"{(1,) + tuple(ehs.shape[1:])}")
        return embeds.to(ehs.dtype).expand(B, -1, -1)

    def _algebra_embeds(self, concepts, ids, embeds, B, ehs):
        """The three concepts' text embeddings [3B, T, ctx], concept-major: each encoded once, repeated over the batch."""
        if embeds is None:
            if ids is None:
                ids = self._tokenize(list(concepts))
            embeds = self.text_encoder(ids.to(self.device))[0]
        embeds = embeds.to(self.device)
        if embeds.dim() != 3 or embeds.shape[0] != 3 or tuple(embeds.shape[1:]) != tuple(ehs.shape[1:]):
            raise ValueError(f"concept-algebra embeddings {tuple(embeds.shape)}: expected three concepts of shape "
                             f"{(3,) + tuple(ehs.shape[1:])}")
        return embeds.to(ehs.dtype)[:, None].expand(3, B, -1, -1).reshape((3 * B,) + tuple(ehs.shape[1:]))

    def _eager_loop(self, latents, ehs, B, shape, cfg_on, guidance_scale, callback, callback_steps, end_iteration=None,
                    sld=None, algebra=False, masks=None):
        dev, sch = self.device, self.scheduler
        was_training = self.unet.training
        self.unet.eval()
        try:
            x2 = torch.empty((5 * B if algebra else 3 * B if sld is not None else 2 * B if cfg_on else B,) + shape[1:],
                             device=dev, dtype=torch.float32)
            if algebra:
                ws = torch.zeros(k.calg_workspace_elems(*shape[:2], shape[2] * shape[3]), device=dev, dtype=torch.float64)
            if sld is not None:
                mom = torch.zeros(shape, device=dev, dtype=torch.float32)
            for i, t in enumerate(sch.timesteps.tolist()[:end_iteration]):
                x2[:B].copy_(latents)
                if cfg_on:
                    x2[B:2 * B].copy_(latents)
                if sld is not None:
                    x2[2 * B:].copy_(latents)
                if algebra:
                    for j in range(2, 5):
                        x2[j * B:(j + 1) * B].copy_(latents)
                tt = torch.full((x2.shape[0],), t, device=dev,
                                dtype=torch.float32 if sch.timesteps.is_floating_point() else torch.int64)
                if masks is not None:                                 # U-Net call i: timestep slot i (PNDM: 0, 0, 1, 2, ...)
                    masks.apply(slot=max(i - 1, 0) if type(sch) is PNDMScheduler else i)
                out = self.unet(sch.scale_model_input(x2, t), tt, ehs, return_dict=False)[0]
                if algebra:       # the two sums over the whole batch, then the projection and the guidance
                    out = out.contiguous()
                    noise = torch.empty(shape, device=dev, dtype=torch.float32)
                    k.calg_dots(out, 1, B, 1, shape[1] * shape[2] * shape[3], ws)
                    k.calg_guidance(out, noise, guidance_scale, ws)
                elif sld is not None:
                    noise = torch.empty(shape, device=dev, dtype=torch.float32)
                    k.sld_guidance(out.contiguous(), noise, mom, guidance_scale, sld, i >= sld.warmup_steps)
                elif cfg_on:      # uncond + g (text - uncond) = (1 - g) uncond + g text, in place on the text half
                    noise = out[B:]
                    k.axpby(out[:B], noise, 1.0 - guidance_scale, guidance_scale)
                else:
                    noise = out
                latents = sch.step(noise.contiguous(), t, latents, return_dict=False)[0]
                if callback is not None and i % callback_steps == 0:
                    callback(i, t, latents)
        finally:
            self.unet.train(was_training)
        return latents

    __call__ = generate_samples
