"""Safe Latent Diffusion, host side (no GPU needed): the presets of configs/baselines/sld.yaml, when SLD is active, the
directory and file names of the reference's baselines/*/eval-scripts/sld-generate-images.py, its prompt CSV and the `_SLD_<type>`
suffix of the evaluation scripts.  The arithmetic is in csrc/sampler.hip (pdmk_sld_*), the loop in
pdm/pipelines/pruning_pipelines.py.
"""
import csv
import os

PRESET_KEYS = ("sld_guidance_scale", "sld_warmup_steps", "sld_threshold", "sld_momentum_scale", "sld_mom_beta")


def settings_path():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "configs", "baselines",
                        "sld.yaml")


def load_settings(path=None):
    """{"safety_concept": str, "presets": {name: {the five PRESET_KEYS}}} of the settings YAML."""
    import yaml
    with open(path or settings_path(), encoding="utf-8") as f:
        settings = yaml.safe_load(f)
    for name, p in settings["presets"].items():
        if sorted(p) != sorted(PRESET_KEYS):
            raise ValueError(f"{path or settings_path()}: preset {name!r} must hold exactly {', '.join(PRESET_KEYS)}")
    return settings


def preset(sld_type, path=None):
    """The five keywords of generate_samples for --sld_type Weak / Medium / Strong / Max; anything else raises."""
    presets = load_settings(path)["presets"]
    if sld_type not in presets:
        raise ValueError(f"--sld_type {sld_type!r}: expected one of {', '.join(presets)}")
    p = presets[sld_type]
    return dict(sld_guidance_scale=float(p["sld_guidance_scale"]), sld_warmup_steps=int(p["sld_warmup_steps"]),
                sld_threshold=float(p["sld_threshold"]), sld_momentum_scale=float(p["sld_momentum_scale"]),
                sld_mom_beta=float(p["sld_mom_beta"]))


def default_concept(path=None):
    return load_settings(path)["safety_concept"]


def sampling_kwargs(sld_type, concept=None, path=None):
    """generate_samples keywords that sample with the preset `sld_type` against `concept` (None: the default sentence)."""
    return dict(preset(sld_type, path), safety_concept=concept if concept is not None else default_concept(path))


def is_active(guidance_scale, sld_guidance_scale, has_concept):
    """diffusers' `enable_safety_guidance = sld_guidance_scale > 1.0 and do_classifier_free_guidance`, and a concept to
    guide away from."""
    return bool(has_concept) and float(sld_guidance_scale) > 1.0 and float(guidance_scale) > 1.0


def folder_path(save_path, sld_type, sld_concept):
    """sld-generate-images.py:24."""
    return f"{save_path}/SLD_{sld_type}_{sld_concept}"


def image_name(case_number, num):
    """sld-generate-images.py:69."""
    return f"{case_number}_{num}.png"


def with_suffix(name, sld_type):
    """A path component of the evaluation scripts: `name` for a plain run, `name_SLD_<type>` for an SLD one."""
    return name if sld_type is None else f"{name}_SLD_{sld_type}"


def sample_cases(pipe, prompts_path, folder, from_case=0, till_case=None, num_samples=1, prompt_kwargs=None, **sampling):
    """The row loop of the reference's sld-generate-images.py and generate-images.py: per row of the prompt CSV
    `torch.Generator(device).manual_seed(evaluation_seed)`, `num_samples` images of the prompt as one batch (`sampling`: the
    keywords of the pipeline call), uint8 as diffusers' numpy_to_pil (rounded), written to <folder>/<case_number>_<n>.png.
    prompt_kwargs: callable(prompt, num_samples) -> the pipeline keywords that stand for the prompt (debias-VL passes
    transformed embeddings); None: `prompt=[prompt] * num_samples`.  Returns the paths written, in order."""
    import torch
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    written = []
    for case_number, prompt, seed in read_cases(prompts_path, from_case, till_case):
        gen = torch.Generator(device=pipe.device).manual_seed(seed)
        text = dict(prompt=[prompt] * num_samples) if prompt_kwargs is None else prompt_kwargs(prompt, num_samples)
        images = pipe(generator=gen, output_type="u8_round", **text, **sampling).images
        for num, im in enumerate(images):
            written.append(os.path.join(folder, image_name(case_number, num)))
            Image.fromarray(im).save(written[-1])
    return written


def read_cases(path, from_case=0, till_case=None):
    """[(case_number, prompt, evaluation_seed)] of the prompt CSV in file order, rows with case_number < from_case (or, with
    till_case, > till_case) left out."""
    cases = []
    with open(path, encoding="utf-8", newline="") as f:
        for row in csv.DictReader(f):
            missing = [c for c in ("case_number", "prompt", "evaluation_seed") if c not in row]
            if missing:
                raise ValueError(f"{path}: expected the columns `case_number`, `prompt` and `evaluation_seed`, "
                                 f"got {sorted(k for k in row if k)}")
            case = int(row["case_number"])
            if case < int(from_case) or (till_case is not None and case > int(till_case)):
                continue
            cases.append((case, str(row["prompt"]), int(row["evaluation_seed"])))
    return cases
