"""Concept algebra, host side (no GPU needed): the flag rules and paths of the reference's
baselines/unified-concept-editing/eval-scripts/concept_algebra.py and the argument rules of generate_samples' `algebra_*`
keywords.  The arithmetic is in csrc/sampler.hip (pdmk_calg_*), the loop in pdm/pipelines/pruning_pipelines.py.
"""
import os

DEFAULT_CONCEPTS = "a man,a woman,a person"


def split_concepts(text):
    """`--concepts_to_project`: comma separated, stripped; anything but three raises (the reference raises a string there)."""
    concepts = [c.strip() for c in str(text).split(",")]
    if len(concepts) != 3:
        raise ValueError(f"--concepts_to_project {text!r}: must provide 3 concepts to project, comma separated")
    return concepts


def count_concepts(concepts):
    """How many concepts `concepts` holds: a list of strings, [n, T] token ids or [n, T, ctx] embeddings."""
    if isinstance(concepts, str):
        return 1
    shape = getattr(concepts, "shape", None)
    return len(concepts) if shape is None else (int(shape[0]) if len(shape) > 1 else 1)


def check_sampling(guidance_scale, with_sld, concepts):
    """The rules of generate_samples(algebra_concepts= | algebra_ids= | algebra_embeds=): the projection acts on the text
    branch of classifier-free guidance, so it needs guidance_scale > 1; its five row blocks exclude SLD's three; exactly three
    concepts (p0, p1 span the direction, p2 is the reference point)."""
    if with_sld:
        raise ValueError("concept algebra and Safe Latent Diffusion cannot be combined: pass algebra_* or safety_concept*, "
                         "not both")
    if not float(guidance_scale) > 1.0:
        raise ValueError(f"concept algebra needs classifier-free guidance: guidance_scale={guidance_scale} must be > 1")
    n = count_concepts(concepts)
    if n != 3:
        raise ValueError(f"concept algebra takes exactly three concepts, got {n}")


def folder_path(save_path, model_name):
    """concept_algebra.py:35 / debiasing_vl.py:56, of the last path component when --model_name is a file path."""
    name = os.path.basename(model_name.rstrip("/")) or model_name
    return f'{save_path}/{name.replace("diffusers-", "").replace(".pt", "")}'


def erasure_checkpoint(model_name, models_dir):
    """None for `original`; else the file to lay over the pruned checkpoint (FileNotFoundError naming both places tried)."""
    if model_name == 'original':
        return None
    for path in (model_name, os.path.join(models_dir, model_name)):
        if os.path.exists(path):
            return path
    raise FileNotFoundError(f"--model_name {model_name}: neither {model_name} nor {os.path.join(models_dir, model_name)} exists")


def add_common_arguments(parser):
    """The flags concept_algebra.py and debiasing_vl.py share with generate-images.py, then the local-loading flags of
    scripts/baselines/unified_concept_editing/generate_images.py."""
    parser.add_argument('--model_name', help='name of model', type=str, required=True)
    parser.add_argument('--prompts_path', help='path to csv file with prompts', type=str, required=True)
    parser.add_argument('--save_path', help='folder where to save images', type=str, required=True)
    parser.add_argument('--device', help='cuda device to run on', type=str, required=False, default='cuda:0')
    parser.add_argument('--guidance_scale', help='guidance to run eval', type=float, required=False, default=7.5)
    parser.add_argument('--image_size', help='image size used to train', type=int, required=False, default=512)
    parser.add_argument('--till_case', help='continue generating from case_number', type=int, required=False, default=1000000)
    parser.add_argument('--from_case', help='continue generating from case_number', type=int, required=False, default=0)
    parser.add_argument('--num_samples', help='number of samples per prompt', type=int, required=False, default=1)
    parser.add_argument('--ddim_steps', help='ddim steps of inference used to train', type=int, required=False, default=100)
    parser.add_argument('--models_dir', type=str, default='models', help="where --model_name is looked up when it is not a file")
    parser.add_argument('--base_config_path', type=str, default=None)
    parser.add_argument('--model_id', type=str, default='stabilityai/stable-diffusion-2-1')
    parser.add_argument('--ckpt_path', type=str, default=None, help="the pruned checkpoint directory: arch_vector.pt + unet/")
    parser.add_argument('--mixed_precision', type=str, default=None, choices=["no", "bf16"])
    parser.add_argument('--tiny', action="store_true", help="tiny U-Net topology (tests)")
    parser.add_argument('--scheduler', type=str, default='pndm', choices=["pndm", "lms"],
                        help="sampler: the project's PNDM (default) or the reference's K-LMS (LMSDiscreteScheduler)")
    return parser


def load_pipeline(args):
    """(FrozenModels, pipeline) of the common flags: the pruned checkpoint --ckpt_path, with the erasure checkpoint
    --model_name laid over it unless that is `original`."""
    import torch
    from .load_models import FrozenModels, cuda_device, inference_config
    if args.ckpt_path is None:
        raise ValueError("--ckpt_path is required (the pruned checkpoint directory: arch_vector.pt + unet/)")
    device = torch.device(args.device)
    if device.type != "cuda":
        raise ValueError(f"--device {args.device}: the samplers run on the GPU only")
    erasure = erasure_checkpoint(args.model_name, args.models_dir)
    config = inference_config(args.base_config_path, args.model_id, args.tiny, args.mixed_precision)
    models = FrozenModels(config, cuda_device(device.index or 0))
    unet = models.load_unet(args.ckpt_path)
    if erasure is not None:
        from .erasure_utils import load_erasure_checkpoint
        load_erasure_checkpoint(unet, erasure)
    return models, models.pipeline(unet, kind=getattr(args, "scheduler", "pndm"))
