"""Object erasure on Imagenette: erase one of ten ImageNet classes, sample `an image of a <class>`, classify the images with
ResNet-50 - accuracy on the erased class should fall, accuracy on the other nine should stay.  The host side of the
reference's two scripts, baselines/unified-concept-editing/eval-scripts/imageclassify.py (the same file under
baselines/erasing/oldcode_erasing_compvis/eval-scripts) and baselines/concept_prune/benchmarking/object_erase.py; the
classifier is pdm/models/resnet (pdmk_conv2d_fwd_res, pdmk_softmax_topk).

No GPU needed for: the file listing and case numbers, the inner join of the prompts frame with the per-image results (what
`pd.merge` does there), the CSV, the Imagenette table (configs/baselines/imagenette.yaml), the row selection and the result
paths.  GPU side: `classify_folder`, `generate`, `score_folder`.  Nothing here imports pandas or torchvision.
"""
import csv
import json
import os

import numpy as np

from .perceptual import read_frame, write_frame


# ---- the Imagenette table and category names
def imagenette_path():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "configs", "baselines",
                        "imagenette.yaml")


def imagenette_classes(path=None):
    """{class name: ImageNet-1k index} in the file's order."""
    import yaml
    with open(path or imagenette_path(), encoding="utf-8") as f:
        table = yaml.safe_load(f)["classes"]
    return {str(name): int(index) for name, index in table.items()}


def label_index(label, classes=None):
    """The ImageNet index of a prompt CSV label, case-insensitive; an unknown label raises ValueError naming it."""
    classes = classes if classes is not None else imagenette_classes()
    by_lower = {name.lower(): index for name, index in classes.items()}
    if str(label).lower() not in by_lower:
        raise ValueError(f"label {label!r} is not an Imagenette class ({', '.join(classes)})")
    return by_lower[str(label).lower()]


def load_categories(path):
    """The 1000 ImageNet category names, one per line (torchvision's `weights.meta["categories"]` written out)."""
    with open(path, encoding="utf-8") as f:
        names = [line.rstrip("\r\n") for line in f]
    while names and names[-1] == "":
        names.pop()
    if len(names) != 1000:
        raise ValueError(f"{path}: expected 1000 category names, one per line, got {len(names)}")
    return names


def category_name(index, categories=None, classes=None):
    """`categories[index]` with a categories file; without one the Imagenette name where the index is one of the ten,
    otherwise the index as text."""
    if categories is not None:
        return categories[int(index)]
    classes = classes if classes is not None else imagenette_classes()
    for name, i in classes.items():
        if i == int(index):
            return name
    return str(int(index))


# ---- imageclassify.py: names, the join, the CSV
def image_names(folder):
    """Names containing `.png` or `.jpg`, sorted (the reference keeps os.listdir order, which no two machines share)."""
    return sorted(n for n in os.listdir(folder) if ".png" in n or ".jpg" in n)


def case_number(name):
    """imageclassify.py:75: `10_0.png` -> 10."""
    return int(name.split("/")[-1].split("_")[0].replace(".png", "").replace(".jpg", ""))


def classification_columns(topk):
    return [f"{c}_top{k}" for k in range(1, int(topk) + 1) for c in ("category", "index", "scores")]


def classification_rows(names, probs, idx, categories=None):
    """One row per image: case_number, then per k the category, the index and the score (an fp32 scalar: the CSV shows its
    shortest float32 digits, as pandas writes a float32 column)."""
    classes = imagenette_classes()
    probs, idx = np.asarray(probs, np.float32), np.asarray(idx, np.int64)
    rows = []
    for n, p, j in zip(names, probs, idx):
        row = [case_number(n)]
        for k in range(len(j)):
            row += [category_name(j[k], categories, classes), int(j[k]), p[k]]
        rows.append(row)
    return rows


def merge_on_case_number(header, rows, result_header, result_rows):
    """`pd.merge(df, df_results)`: the inner join on `case_number` (the only shared column), the prompt frame's columns
    first and its row order kept, the results of one case in their own order.  A case without images and an image without a
    prompt row drop out; three images of a case give three rows."""
    ci, ri = header.index("case_number"), result_header.index("case_number")
    by_case = {}
    for r in result_rows:
        by_case.setdefault(int(r[ri]), []).append([v for i, v in enumerate(r) if i != ri])
    out = []
    for row in rows:
        left = list(row)
        left[ci] = int(float(left[ci]))                    # df['case_number'].astype('int')
        for right in by_case.get(left[ci], []):
            out.append(left + right)
    return list(header) + [c for i, c in enumerate(result_header) if i != ri], out


def default_save_path(folder):
    """<folder>/<basename(folder)>_classification.csv (the reference's default names an undefined variable and raises)."""
    return os.path.join(folder, f"{os.path.basename(os.path.normpath(folder))}_classification.csv")


def classify_folder(folder, prompts_path, save_path, model, topk=5, batch_size=250, categories=None, resize_size=232,
                    crop_size=224):
    """imageclassify.py over a folder: the CSV at save_path, and (header, rows) as written."""
    names = image_names(folder)
    if not names:
        raise ValueError(f"{folder}: no .png / .jpg images")
    probs, idx = model.classify([os.path.join(folder, n) for n in names], topk=topk, resize_size=resize_size, crop_size=crop_size,
                                batch_size=max(1, min(int(batch_size), len(names))))
    header, rows = read_frame(prompts_path)
    res_header = ["case_number"] + classification_columns(topk)
    out_header, out_rows = merge_on_case_number(header, rows, res_header, classification_rows(names, probs.numpy(), idx.numpy(),
                                                                                              categories))
    write_frame(save_path, out_header, out_rows)
    return out_header, out_rows


# ---- object_erase.py: rows, paths
def read_prompt_rows(path):
    """The rows of the Imagenette prompt CSV as dicts; `prompt`, `evaluation_seed` and `class` (or `label_str`) are needed."""
    with open(path, encoding="utf-8", newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows:
        raise ValueError(f"{path}: no rows")
    have = set(rows[0])
    if not {"prompt", "evaluation_seed"} <= have or not ({"class", "label_str"} & have):
        raise ValueError(f"{path}: expected the columns `prompt`, `evaluation_seed` and `class` (or `label_str`), got {sorted(have)}")
    return rows


def select_rows(rows, target, removal_mode, dbg=False):
    """[(prompt, evaluation_seed, lower-case label)]: `erase` the rows of the target class (case-insensitive), `keep` all
    others, each with its own label; dbg: the first 11."""
    if removal_mode not in ("erase", "keep"):
        raise ValueError(f"--removal_mode {removal_mode!r}: expected erase or keep")
    col = "class" if "class" in rows[0] else "label_str"
    want = str(target).lower()
    out = [(r["prompt"], int(r["evaluation_seed"]), r[col].lower()) for r in rows if (r[col].lower() == want) == (removal_mode == "erase")]
    return out[:11] if dbg else out


def result_dir(args):
    """<root>/<model>/<target>/<baseline>/benchmarking/concept_<mode>: object_erase.py:81-82 with the root and the model
    component of the artist-erasure script (pdm/utils/erasure_utils.py); with --sld_type the baseline is <baseline>_SLD_<type>."""
    from .erasure_utils import model_component, result_root
    from .sld import with_suffix
    return os.path.join(result_root(args.result_dir, args.seed, args.res_path), model_component(args.model_id), args.target,
                        with_suffix(args.baseline, getattr(args, "sld_type", None)), "benchmarking", f"concept_{args.removal_mode}")


def result_name(removal_mode, ckpt_name):
    """object_erase.py:145-146, the reference's `p` as it forms it."""
    p = ckpt_name.split("/")[-1].split(".pt")[0] if ckpt_name is not None else "concept-prune"
    return f"results_{removal_mode}_{p}.json"


def image_file(i):
    return f"removed_{i}.png"


def accuracy(predicted, labels, classes=None):
    """(hits, rows): a hit where the top-1 index is the label's ImageNet index."""
    classes = classes if classes is not None else imagenette_classes()
    want = [label_index(l, classes) for l in labels]
    if len(want) != len(predicted):
        raise ValueError(f"{len(predicted)} predictions for {len(want)} rows")
    return sum(int(p) == w for p, w in zip(predicted, want)), len(want)


def write_result(directory, removal_mode, ckpt_name, hits, rows):
    results = {"average_accuracy": hits / rows}
    path = os.path.join(directory, result_name(removal_mode, ckpt_name))
    with open(path, "w") as f:
        json.dump(results, f)
    return results, path


# ---- GPU side
def generate(selected, directory, pipe, resolution, steps, sld=None, guidance_scale=7.5):
    """removed_{i}.png for row i: `torch.Generator(device).manual_seed(evaluation_seed)`, one image of the prompt, uint8 as
    diffusers' numpy_to_pil (rounded).  sld: the Safe Latent Diffusion keywords of pdm/utils/sld.py sampling_kwargs."""
    import torch
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for i, (prompt, seed, label) in enumerate(selected):
        print(f"Prompt: {prompt}, Seed: {seed}, Label: {label}")
        gen = torch.Generator(device=pipe.device).manual_seed(int(seed))
        im = pipe(prompt=[prompt], generator=gen, num_inference_steps=steps, guidance_scale=guidance_scale, height=resolution,
                  width=resolution, output_type="u8_round", **(sld or {})).images[0]
        Image.fromarray(im).save(os.path.join(directory, image_file(i)))


def score_folder(selected, directory, model, batch_size=64, resize_size=232, crop_size=224, with_predictions=False):
    """(hits, rows) over removed_0.png .. of `directory`, one per selected row; a missing file raises.  with_predictions:
    (hits, rows, the top-1 index of every image)."""
    paths = [os.path.join(directory, image_file(i)) for i in range(len(selected))]
    missing = [os.path.basename(p) for p in paths if not os.path.isfile(p)]
    if missing:
        raise ValueError(f"{directory}: {len(selected)} rows, {len(missing)} images missing (first: {missing[:3]})")
    _, idx = model.classify(paths, topk=1, resize_size=resize_size, crop_size=crop_size, batch_size=batch_size)
    predicted = idx[:, 0].tolist()
    hits, rows = accuracy(predicted, [label for _, _, label in selected])
    return (hits, rows, predicted) if with_predictions else (hits, rows)
