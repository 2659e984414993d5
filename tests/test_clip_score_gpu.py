"""The CLIP-score scripts end to end (-m gpu): save_captions -> clip_features -> clip_score `main()`s on a temp tree of 12
seeded `.npy` images (mixed sizes, 512 x 512 among them) and their captions, with the tiny transformers-layout model of
tests/clip_score_fixtures.py, against the score transformers + PIL compute (tests/golden/clip_score_hf.npz)."""
import importlib.util
import os

import numpy as np
import pytest

import clip_score_fixtures as fx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "clip_score_hf.npz"))
LOGIT_SCALE = 1 / 0.07


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "unlearn-ft_amd", "scripts", "metrics", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("clipscore"))
    model = fx.write_hf_dir(root, "tiny")
    ann, images = fx.write_e2e_tree(root)
    caps = _script("save_captions").main(["--annotations_file", ann])
    feats = _script("clip_features").main(["--dataset_path", caps, "--clip_model", model, "--num_workers", "0",
                                            "--batch_size", "5"])
    return dict(root=root, model=model, images=images, caps=caps, feats=feats)


def test_features_unit_norm_and_match(tree):
    files = sorted(os.listdir(tree["feats"]))
    assert files == ["COCO_val2014_tiny_%012d.npy" % (i + 1) for i in range(12)]
    assert os.path.basename(tree["feats"]) == "clip-tiny_clip_features"
    f = np.stack([np.load(os.path.join(tree["feats"], n)) for n in files])
    assert f.dtype == np.float32 and f.shape == GOLD["e2e_txt"].shape
    assert np.abs(np.linalg.norm(f, axis=1) - 1).max() < 1e-5
    assert np.abs(f - GOLD["e2e_txt"]).max() < 3e-4


def test_score_and_result_line(tree):
    res = os.path.join(tree["root"], "results")
    argv = ["--gen_images_dir", tree["images"], "--text_features_dir", tree["feats"], "--clip_model", tree["model"],
            "--result_dir", res, "--dataset_name", "coco", "--num_workers", "0"]
    mod = _script("clip_score")
    s1 = mod.main(argv)
    assert abs(s1 - float(GOLD["e2e_score"])) <= 1e-3 * LOGIT_SCALE, (s1, float(GOLD["e2e_score"]))
    s2 = mod.main(argv)
    with open(os.path.join(res, "clip_score_coco.txt")) as f:
        assert f.read() == f"{tree['images']} {s1}\n{tree['images']} {s2}\n"


def test_batch_sizes_and_workers_agree(tree):
    from pdm.models.clip.clip_model import CLIPModel
    from pdm.utils.clip_utils import clip_score
    m = CLIPModel.from_pretrained(tree["model"])
    scores = [clip_score(tree["feats"], tree["images"], num_workers=w, batch_size=b, model=m)
              for b, w in [(64, 0), (1, 0), (5, 2), (64, 2)]]
    # relative to the score's scale, logit_scale.exp() (random weights put this score itself near 0)
    assert max(scores) - min(scores) <= 1e-5 * LOGIT_SCALE, scores


def test_missing_image_raises(tree, tmp_path):
    import shutil
    from pdm.utils.clip_utils import clip_score
    sub = str(tmp_path / "gen")
    shutil.copytree(tree["images"], sub)
    os.remove(os.path.join(sub, sorted(os.listdir(sub))[3]))
    with pytest.raises(ValueError, match="11 images, 12 text features"):
        clip_score(tree["feats"], sub, clip_model=tree["model"], num_workers=0)
