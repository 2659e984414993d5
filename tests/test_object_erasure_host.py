"""pdm/utils/object_erasure.py without a GPU: file listing and case numbers, the inner join of the prompts frame with the
per-image results, the CSV text, the Imagenette table against the shipped prompt CSV, the erase / keep row selection and the
result paths of scripts/metrics/object_erase.py."""
import argparse
import os

import numpy as np
import pytest

from pdm.utils import object_erasure as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSV = os.path.join(ROOT, "tests", "golden", "object_erasure", "imagenette.csv")


def test_image_names_and_case_numbers(tmp_path):
    for n in ("10_0.png", "1_0.png", "2_1.jpg", "2_0.jpg", "notes.txt", "1_0.png.json", "3.png", "7_2.jpeg"):
        (tmp_path / n).write_bytes(b"")
    names = O.image_names(str(tmp_path))
    assert names == ["10_0.png", "1_0.png", "1_0.png.json", "2_0.jpg", "2_1.jpg", "3.png"]      # `in`, as the reference; sorted
    assert [O.case_number(n) for n in ("10_0.png", "1_0.png", "2_1.jpg", "3.png", "a/b/12_4.png")] == [10, 1, 2, 3, 12]
    assert O.case_number("10_0.png") != O.case_number("1_0.png")
    with pytest.raises(ValueError):
        O.case_number("removed_3.png")


def test_merge_is_pandas_inner_join():
    header = ["case_number", "prompt", "class", "evaluation_seed"]
    rows = [["0", "an image of a tench", "tench", "11"], ["1", "an image of a church", "church", "12"],
            ["2", "an image of a parachute", "parachute", "13"], ["3.0", "an image of a tench", "tench", "14"]]
    res_header = ["case_number", "category_top1", "index_top1", "scores_top1"]
    res_rows = [[2, "parachute", 701, 0.5], [0, "tench", 0, 0.25], [9, "church", 497, 0.1], [2, "701", 3, 0.125], [2, "x", 4, 0.75],
                [3, "tench", 0, 1.0]]
    h, out = O.merge_on_case_number(header, rows, res_header, res_rows)
    assert h == header + res_header[1:]
    # case 1 has no image and drops out, the image of case 9 has no prompt row and drops out, case 2 has three images
    assert out == [[0, "an image of a tench", "tench", "11", "tench", 0, 0.25],
                   [2, "an image of a parachute", "parachute", "13", "parachute", 701, 0.5],
                   [2, "an image of a parachute", "parachute", "13", "701", 3, 0.125],
                   [2, "an image of a parachute", "parachute", "13", "x", 4, 0.75],
                   [3, "an image of a tench", "tench", "14", "tench", 0, 1.0]]


def test_classification_csv_text(tmp_path):
    names = ["1_0.png", "10_0.png", "10_1.jpg"]
    probs = np.array([[0.75, 0.125], [0.1, 0.05], [0.3, 0.2]], np.float32)
    idx = np.array([[497, 3], [0, 701], [999, 574]])
    assert O.classification_columns(2) == ["category_top1", "index_top1", "scores_top1", "category_top2", "index_top2", "scores_top2"]
    res = O.classification_rows(names, probs, idx)
    h, out = O.merge_on_case_number(["case_number", "prompt"], [["1", "a, b"], ["10", "c"]], ["case_number"] + O.classification_columns(2), res)
    from pdm.utils.perceptual import write_frame
    path = write_frame(str(tmp_path / "sub" / "out.csv"), h, out)
    with open(path, encoding="utf-8", newline="") as f:
        text = f.read()
    assert text == (",case_number,prompt,category_top1,index_top1,scores_top1,category_top2,index_top2,scores_top2\r\n"
                    "0,1,\"a, b\",church,497,0.75,3,3,0.125\r\n"
                    "1,10,c,tench,0,0.1,parachute,701,0.05\r\n"
                    "2,10,c,999,999,0.3,golf ball,574,0.2\r\n")
    cats = [f"name {i}" for i in range(1000)]
    assert O.classification_rows(names[:1], probs[:1], idx[:1], cats)[0][:4] == [1, "name 497", 497, np.float32(0.75)]
    assert O.default_save_path("/a/b/run7") == "/a/b/run7/run7_classification.csv"
    assert O.default_save_path("/a/b/run7/") == "/a/b/run7/run7_classification.csv"


def test_load_categories(tmp_path):
    p = tmp_path / "cats.txt"
    p.write_text("".join(f"class {i}\n" for i in range(1000)), encoding="utf-8")
    cats = O.load_categories(str(p))
    assert len(cats) == 1000 and cats[0] == "class 0" and cats[999] == "class 999"
    p.write_text("".join(f"class {i}\n" for i in range(999)), encoding="utf-8")
    with pytest.raises(ValueError, match="1000"):
        O.load_categories(str(p))


def test_imagenette_table_matches_the_prompt_csv():
    classes = O.imagenette_classes()
    assert len(classes) == 10 and len(set(classes.values())) == 10
    assert classes == {"tench": 0, "English springer": 217, "cassette player": 482, "chain saw": 491, "church": 497,
                       "French horn": 566, "garbage truck": 569, "gas pump": 571, "golf ball": 574, "parachute": 701}
    rows = O.read_prompt_rows(CSV)
    assert len(rows) == 5000
    assert sorted({r["class"] for r in rows}) == sorted(classes)
    assert all(r["prompt"].startswith("an image of a") and r["class"].lower() in r["prompt"].lower() for r in rows)
    assert len({(r["prompt"], r["class"]) for r in rows}) == 10                 # one prompt per class, 500 seeds each
    assert O.label_index("french HORN") == 566 and O.category_name(566) == "French horn" and O.category_name(5) == "5"
    with pytest.raises(ValueError, match="goldfish"):
        O.label_index("goldfish")


def test_erase_keep_selection():
    rows = O.read_prompt_rows(CSV)
    erase = O.select_rows(rows, "Church", "erase")
    keep = O.select_rows(rows, "Church", "keep")
    assert len(erase) == 500 and len(keep) == 4500
    assert {l for _, _, l in erase} == {"church"} and "church" not in {l for _, _, l in keep}
    assert len({l for _, _, l in keep}) == 9 and all(l == l.lower() for _, _, l in keep)
    first = next(r for r in rows if r["class"] == "church")
    assert erase[0] == ("an image of a church", int(first["evaluation_seed"]), "church")
    assert keep[0] == (rows[0]["prompt"], int(rows[0]["evaluation_seed"]), "tench")
    assert len(O.select_rows(rows, "church", "keep", dbg=True)) == 11 and O.select_rows(rows, "church", "erase", dbg=True) == erase[:11]
    alt = [{"prompt": r["prompt"], "evaluation_seed": r["evaluation_seed"], "label_str": r["class"]} for r in rows[:600]]
    assert len(O.select_rows(alt, "tench", "erase")) == 500 and len(O.select_rows(alt, "tench", "keep")) == 100
    with pytest.raises(ValueError):
        O.select_rows(rows, "church", "remove")


def test_accuracy_counts_index_hits():
    assert O.accuracy([497, 0, 497, 701], ["church", "church", "tench", "parachute"]) == (2, 4)
    with pytest.raises(ValueError):
        O.accuracy([1], ["church", "tench"])


def test_result_paths_and_p_rule(tmp_path):
    a = argparse.Namespace(result_dir=None, seed=3, res_path="results/results_seed_0/stable-diffusion", model_id="CompVis/stable-diffusion-v1-4",
                           target="church", baseline="uce", removal_mode="erase", sld_type=None)
    assert O.result_dir(a) == "results/results_seed_3/stable-diffusion/CompVis/stable-diffusion-v1-4/church/uce/benchmarking/concept_erase"
    snap = tmp_path / "snapshot"
    snap.mkdir()
    a = argparse.Namespace(result_dir=str(tmp_path / "res"), seed=0, res_path="x", model_id=str(snap), target="gas pump", baseline="pdm",
                           removal_mode="keep", sld_type="Max")
    assert O.result_dir(a) == os.path.join(str(tmp_path / "res"), "snapshot", "gas pump", "pdm_SLD_Max", "benchmarking", "concept_keep")
    assert O.result_name("erase", None) == "results_erase_concept-prune.json"
    assert O.result_name("keep", "runs/uce/erased-church.pt") == "results_keep_erased-church.json"
    assert O.result_name("erase", "runs/bilevel/checkpoint-9") == "results_erase_checkpoint-9.json"
    assert O.result_name("erase", "runs/bilevel/checkpoint-9/") == "results_erase_.json"          # the reference's split('/')[-1]
    assert O.image_file(12) == "removed_12.png"
    results, path = O.write_result(str(tmp_path), "erase", "a/b.pt", 1, 4)
    assert results == {"average_accuracy": 0.25} and os.path.basename(path) == "results_erase_b.json"
    with open(path) as f:
        assert f.read() == '{"average_accuracy": 0.25}'
