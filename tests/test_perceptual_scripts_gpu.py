"""scripts/baselines/unified_concept_editing/{lpips_eval,styleloss,generate_images}.py end to end (-m gpu): two folders of
`<case>_<n>.png` files with weights read from files, against the restatements of tests/perceptual_fixtures.py; and the plain
generator on the tiny snapshot and 2-step checkpoint of tests/test_fid_images_gpu.py."""
import csv
import importlib.util
import math
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import perceptual_fixtures as fx  # noqa: E402
import test_fid_images_gpu as fid_test            # its fixture tree and 2-step training run (_setup)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["1_0.png", "1_1.png", "1_2.png", "2_0.png", "10_0.png"]
MISSING = "1_1.png"                               # not in the edited folder
CASES = [1, 2, 10, 3]                             # 3 has no files


def _script(name):
    path = os.path.join(ROOT, "unlearn-ft_amd", "scripts", "baselines", "unified_concept_editing", name + ".py")
    spec = importlib.util.spec_from_file_location(name + "_perceptual_gpu", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("perceptual_scripts")
    a, b = fx.pairs(50, len(FILES), 96)
    imgs = {}
    for d in ("original", "erased-model"):
        (root / d).mkdir()
    for n, x, y in zip(FILES, a, b):
        Image.fromarray(x).save(root / "original" / n)
        if n != MISSING:
            Image.fromarray(y).save(root / "erased-model" / n)
            imgs[n] = (x, y)
    with open(root / "prompts.csv", "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["case_number", "prompt", "evaluation_seed"])
        for c in CASES:
            w.writerow([c, f"prompt, number {c}", 1000 + c])
    torch.save(fx.vgg_state_dict(), root / "vgg19.pth")
    torch.save(fx.alexnet_state_dict(), root / "alexnet.pth")
    torch.save(fx.lin_state_dict(), root / "alex.pth")
    return dict(root=str(root), imgs=imgs, owner={1: ["1_0.png", "1_2.png"], 2: ["2_0.png"], 10: ["10_0.png"], 3: []})


def _read(path):
    with open(path, encoding="utf-8", newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def _case_means(folders, per_file):
    """{case: mean over its files} of a {file: value(s)} table."""
    return {c: np.mean([per_file[n] for n in names], axis=0) for c, names in folders["owner"].items() if names}


def _argv(folders, save="out"):
    r = folders["root"]
    return ["--original_path", os.path.join(r, "original"), "--edited_path", os.path.join(r, "erased-model") + "/",
            "--csv_path", os.path.join(r, "prompts.csv"), "--save_path", os.path.join(r, save)]


def test_lpips_eval(dev, folders, capsys):
    mod = _script("lpips_eval")
    r = folders["root"]
    weights = ["--alexnet_weights", os.path.join(r, "alexnet.pth"), "--lpips_weights", os.path.join(r, "alex.pth")]
    out = mod.main(_argv(folders) + weights + ["--batch_size", "3"])
    assert out == os.path.join(r, "out", "erased-model_lpipsloss.csv") and os.listdir(os.path.join(r, "out")) == ["erased-model_lpipsloss.csv"]
    assert f"{MISSING}: No File" in capsys.readouterr().out
    header, rows = _read(out)
    assert header == ["", "case_number", "prompt", "evaluation_seed", "lpips_loss"]
    assert [row[:4] for row in rows] == [[str(i), str(c), f"prompt, number {c}", str(1000 + c)] for i, c in enumerate(CASES)]
    names = sorted(folders["imgs"])
    a, b = [folders["imgs"][n][0] for n in names], [folders["imgs"][n][1] for n in names]
    sd, lin = fx.alexnet_state_dict(), fx.lin_state_dict()
    ref, cpu32 = ({c: v for c, v in _case_means(folders, dict(zip(names, fx.lpips(sd, lin, a, b, 64, d)))).items()}
                  for d in (torch.float64, torch.float32))
    got = {int(row[1]): float(row[4]) for row in rows}
    assert math.isnan(got[3])
    assert not fx.yardstick([ref[c] for c in (1, 2, 10)], [cpu32[c] for c in (1, 2, 10)], [got[c] for c in (1, 2, 10)], "lpips_eval")
    # --image: one pair, `filename, lpips_loss`
    one = os.path.join(r, "one_lpips.csv")
    v = mod.main(["--original_path", os.path.join(r, "original", "2_0.png"), "--edited_path", os.path.join(r, "erased-model", "2_0.png"),
                  "--image", "--save_path", one] + weights)
    header, rows = _read(one)
    assert header == ["", "filename", "lpips_loss"] and rows == [["0", "2_0.png", repr(v)]]
    assert not fx.yardstick([ref[2]], [cpu32[2]], [v], "lpips_eval --image")
    with pytest.raises(FileNotFoundError, match="alexnet-owt-7be5be79.pth"):
        mod.main(_argv(folders) + ["--alexnet_weights", os.path.join(r, "absent.pth"), "--lpips_weights", os.path.join(r, "alex.pth")])


def test_styleloss(dev, folders, capsys):
    mod = _script("styleloss")
    r = folders["root"]
    weights = ["--vgg_weights", os.path.join(r, "vgg19.pth"), "--imsize", "48"]
    out = mod.main(_argv(folders, "out_style") + weights + ["--batch_size", "3"])
    assert out == os.path.join(r, "out_style", "erased-model_styleloss.csv")
    assert f"{MISSING}: No File" in capsys.readouterr().out
    header, rows = _read(out)
    assert header == ["", "case_number", "prompt", "evaluation_seed", "style_loss", "content_loss", "total_loss"]
    names = sorted(folders["imgs"])
    a, b = [folders["imgs"][n][0] for n in names], [folders["imgs"][n][1] for n in names]
    sd = fx.vgg_state_dict()
    ref, cpu32 = (_case_means(folders, dict(zip(names, fx.vgg_losses(sd, a, b, 48, d)))) for d in (torch.float64, torch.float32))
    assert [int(row[1]) for row in rows] == CASES
    got = {int(row[1]): [float(x) for x in row[4:]] for row in rows}
    assert all(math.isnan(x) for x in got[3])
    for j, name in enumerate(("style", "content", "total")):
        assert not fx.yardstick([ref[c][j] for c in (1, 2, 10)], [cpu32[c][j] for c in (1, 2, 10)], [got[c][j] for c in (1, 2, 10)],
                                f"styleloss {name}")
    one = os.path.join(r, "one_style.csv")
    v = mod.main(["--original_path", os.path.join(r, "original", "10_0.png"), "--edited_path",
                  os.path.join(r, "erased-model", "10_0.png"), "--image", "--save_path", one] + weights)
    header, rows = _read(one)
    assert header == ["", "filename", "Style_Loss", "Content_Loss", "Total_Loss"] and rows == [["0", "10_0.png"] + [repr(x) for x in v]]
    for j, name in enumerate(("style", "content", "total")):
        assert not fx.yardstick([ref[10][j]], [cpu32[10][j]], [v[j]], f"styleloss --image {name}")


# ---------------------------------------------------------------------------------------------- generate_images.py
def test_generate_images(dev, tmp_path):
    from PIL import Image
    from pdm.utils.load_models import FrozenModels, inference_config
    mod = _script("generate_images")
    path, ck2, snap = fid_test._setup(tmp_path, bs=2)
    prompts = os.path.join(str(tmp_path), "prompts.csv")
    texts = {0: "a red thing", 1: "the blue one", 2: "and a third", 5: "never sampled"}
    with open(prompts, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["case_number", "prompt", "evaluation_seed"])
        for c, t in texts.items():
            w.writerow([c, t, 1000 + c])

    def argv(save):
        return ["--model_name", "original", "--prompts_path", prompts, "--save_path", save, "--from_case", "1", "--till_case", "2",
                "--num_samples", "2", "--ddim_steps", "2", "--image_size", "64", "--base_config_path", path, "--model_id", snap,
                "--ckpt_path", ck2, "--tiny"]

    save = os.path.join(str(tmp_path), "gen")
    written = mod.main(argv(save))
    folder = os.path.join(save, "original")
    names = [f"{c}_{n}.png" for c in (1, 2) for n in range(2)]
    assert sorted(os.listdir(save)) == ["original"] and sorted(os.listdir(folder)) == names
    assert written == [os.path.join(folder, n) for n in names]
    again = os.path.join(str(tmp_path), "gen2")
    mod.main(argv(again))
    for n in names:
        assert open(os.path.join(folder, n), "rb").read() == open(os.path.join(again, "original", n), "rb").read(), n
    models = FrozenModels(inference_config(path, snap, True, None), dev)
    pipe = models.pipeline(models.load_unet(ck2))
    for c in (1, 2):
        want = pipe(prompt=[texts[c]] * 2, generator=torch.Generator(device=dev).manual_seed(1000 + c), num_inference_steps=2,
                    guidance_scale=7.5, height=64, width=64, output_type="u8_round").images
        assert want.shape == (2, 64, 64, 3) and not np.array_equal(want[0], want[1])
        for n in range(2):
            with Image.open(os.path.join(folder, f"{c}_{n}.png")) as im:
                assert im.format == "PNG" and im.mode == "RGB" and np.array_equal(np.asarray(im), want[n]), (c, n)
    assert mod.folder_path("out", "diffusers-VanGogh-ESDx1-UNET.pt") == "out/VanGogh-ESDx1-UNET"
    with pytest.raises(FileNotFoundError, match="no-such-edit.pt"):
        mod.main(["--model_name", "no-such-edit.pt"] + argv(save)[2:])
