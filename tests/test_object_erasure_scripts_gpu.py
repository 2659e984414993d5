"""The two object-erasure scripts end to end (-m gpu): scripts/baselines/unified_concept_editing/imageclassify.py over a folder
of seeded images with seeded ResNet-50 weights from a file, and scripts/metrics/object_erase.py on the tiny U-Net topology in
both removal modes."""
import csv
import importlib.util
import json
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_fixtures as fx  # noqa: E402
import test_fid_images_gpu as fid_test            # noqa: E402  its fixture tree and 2-step training run (_setup)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = dict(resize_size=36, crop_size=32)
SIZE_ARGV = ["--resize_size", "36", "--crop_size", "32"]


def _script(*parts):
    spec = importlib.util.spec_from_file_location(parts[-1] + "_gpu", os.path.join(ROOT, "unlearn-ft_amd", "scripts", *parts) + ".py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    """Seeded full ResNet-50 weights in a .pth file, and the classifier loaded from it."""
    from pdm.models.resnet import ResNet50Classifier
    path = str(tmp_path_factory.mktemp("resnet") / "resnet50-seeded.pth")
    torch.save(fx.calibrated_state_dict(fx.FULL), path)
    return path, ResNet50Classifier.from_pretrained(path)


# ---------------------------------------------------------------------------------------------- imageclassify.py
NAMES = ["0_0.png", "1_0.png", "10_0.png", "10_1.png", "2_0.jpg", "7_0.png", "3_0.png"]      # case 7 has no prompt row


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("classify")
    d = root / "edited-run"
    d.mkdir()
    for i, n in enumerate(NAMES):
        Image.fromarray(fx.image(400 + i, 40, 40)).save(str(d / n), **({"quality": 95} if n.endswith(".jpg") else {}))
    (d / "notes.txt").write_text("not an image")
    prompts = str(root / "prompts.csv")
    with open(prompts, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["case_number", "prompt", "class", "evaluation_seed"])
        for c in (0, 1, 2, 3, 4, 10):                                                        # case 4 has no image
            w.writerow([c, f"an image of thing {c}", "church", 100 + c])
    return str(d), prompts


def _read(path):
    with open(path, encoding="utf-8", newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_imageclassify(dev, weights, folder, tmp_path):
    path, model = weights
    d, prompts = folder
    mod = _script("baselines", "unified_concept_editing", "imageclassify")
    save = str(tmp_path / "out" / "result.csv")
    argv = ["--folder_path", d, "--prompts_path", prompts, "--topk", "3", "--batch_size", "2", "--resnet_weights", path] + SIZE_ARGV
    assert mod.main(argv + ["--save_path", save]) == save            # 7 images in batches of 2: three full ones and a last partial
    header, rows = _read(save)
    cols = [f"{c}_top{k}" for k in (1, 2, 3) for c in ("category", "index", "scores")]
    assert header == ["", "case_number", "prompt", "class", "evaluation_seed"] + cols
    names = sorted(NAMES)
    probs, idx = model.classify([os.path.join(d, n) for n in names], topk=3, batch_size=2, **SIZES)
    by_name = {n: (probs[i].numpy(), idx[i].numpy()) for i, n in enumerate(names)}
    want = ["0_0.png", "1_0.png", "2_0.jpg", "3_0.png", "10_0.png", "10_1.png"]              # prompt order; case 10's files sorted
    assert [r[1] for r in rows] == ["0", "1", "2", "3", "10", "10"] and [r[0] for r in rows] == [str(i) for i in range(6)]
    from pdm.utils import object_erasure as O
    for r, n in zip(rows, want):
        p, j = by_name[n]
        assert r[2] == f"an image of thing {O.case_number(n)}"
        for k in range(3):
            cat, index, score = r[5 + 3 * k:8 + 3 * k]
            assert int(index) == int(j[k]) and np.float32(score) == p[k], (n, k)
            assert cat == O.category_name(j[k])
    # with a categories file the names come from it
    cats = str(tmp_path / "categories.txt")
    with open(cats, "w", encoding="utf-8") as f:
        f.write("".join(f"category {i}\n" for i in range(1000)))
    mod.main(argv + ["--save_path", save, "--categories_file", cats])
    header2, rows2 = _read(save)
    assert header2 == header
    for a, b in zip(rows, rows2):
        for k in range(3):
            assert b[5 + 3 * k] == f"category {a[6 + 3 * k]}" and b[6 + 3 * k:8 + 3 * k] == a[6 + 3 * k:8 + 3 * k]
    # default --save_path
    out = mod.main(argv)
    assert out == os.path.join(d, "edited-run_classification.csv")
    assert _read(out) == (header, rows)
    os.remove(out)


def test_imageclassify_missing_weights(dev, folder, tmp_path):
    d, prompts = folder
    mod = _script("baselines", "unified_concept_editing", "imageclassify")
    with pytest.raises(FileNotFoundError, match="--resnet_weights"):
        mod.main(["--folder_path", d, "--prompts_path", prompts, "--resnet_weights", str(tmp_path / "none.pth")])


# ---------------------------------------------------------------------------------------------- object_erase.py
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("object_erase")
    path, ck2, snap = fid_test._setup(tmp, bs=2)
    prompts = str(tmp / "imagenette4.csv")
    with open(prompts, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["case_number", "prompt", "class", "evaluation_seed"])
        for i, (c, s) in enumerate([("church", 11), ("tench", 12), ("Church", 13), ("golf ball", 14)]):
            w.writerow([i, f"an image of a {c}", c, s])
    return dict(root=str(tmp), yaml=path, ck2=ck2, snap=snap, prompts=prompts)


@pytest.mark.parametrize("mode,n", [("erase", 2), ("keep", 2)])
def test_object_erase_tiny(dev, weights, trained, mode, n):
    from PIL import Image
    from pdm.utils import object_erasure as O
    path, model = weights
    mod = _script("metrics", "object_erase")
    t = trained
    argv = ["--target", "church", "--baseline", "pruned_baseline", "--removal_mode", mode, "--base_config_path", t["yaml"],
            "--model_id", t["snap"], "--original_ckpt", t["ck2"] + "/", "--result_dir", os.path.join(t["root"], "res"),
            "--prompts_csv", t["prompts"], "--image_resolution", "64", "--num_inference_steps", "3", "--tiny", "--seed", "0",
            "--resnet_weights", path, "--batch_size", "3"] + SIZE_ARGV
    d = O.result_dir(mod.parse_args(argv))
    assert d == os.path.join(t["root"], "res", "snapshot", "church", "pruned_baseline", "benchmarking", f"concept_{mode}")
    r1 = mod.main(argv)
    names = [f"removed_{i}.png" for i in range(n)]
    result = f"results_{mode}_concept-prune.json"                      # no --ckpt_name: the reference's name
    assert sorted(os.listdir(d)) == sorted(names + [result])
    for name in names:
        with Image.open(os.path.join(d, name)) as im:
            assert im.size == (64, 64) and im.mode == "RGB" and im.format == "PNG"
    with open(os.path.join(d, result)) as f:
        text = f.read()
    assert json.loads(text) == r1 and list(r1) == ["average_accuracy"]
    if mode == "erase":                                               # the two `church` rows differ only in their evaluation_seed
        a, b = (np.asarray(Image.open(os.path.join(d, name))) for name in names)
        assert not np.array_equal(a, b)
    # the accuracy is the hit count recomputed from the files
    labels = ["church", "church"] if mode == "erase" else ["tench", "golf ball"]
    _, idx = model.classify([os.path.join(d, name) for name in names], topk=1, **SIZES)
    hits = sum(int(j) == O.label_index(l) for j, l in zip(idx[:, 0].tolist(), labels))
    assert r1["average_accuracy"] == hits / n
    # a second run scores the files that are there: nothing is generated again
    mtimes = {name: os.stat(os.path.join(d, name)).st_mtime_ns for name in names}
    r2 = mod.main(argv)
    assert {name: os.stat(os.path.join(d, name)).st_mtime_ns for name in names} == mtimes
    assert r2 == r1
    with open(os.path.join(d, result)) as f:
        assert f.read() == text


def test_object_erase_unknown_target(dev, trained):
    mod = _script("metrics", "object_erase")
    with pytest.raises(ValueError, match="goldfish"):
        mod.main(["--target", "goldfish", "--baseline", "pruned_baseline", "--removal_mode", "erase", "--original_ckpt", trained["ck2"],
                  "--result_dir", os.path.join(trained["root"], "res2")])
