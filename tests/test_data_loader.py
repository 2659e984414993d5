"""Host side of the image-caption loader (pdm/utils/data.py) on the CPU: dataset sources as the reference builds them
(pdm/utils/data_utils.py:12-65, pdm/datasets/coco.py), caption choice, per-epoch order, rank shards, packing, dropped images."""
import os

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("HF_DATASETS_OFFLINE", "1")

import numpy as np
import pytest
import torch

import data_fixtures as F


def _loader(rows, **kw):
    from pdm.utils.data import ImageCaptionLoader
    return ImageCaptionLoader(rows, **{"batch_size": 2, "resolution": 32, **kw})


@pytest.mark.parametrize("year,split,name", [("2017", "train2017", "%012d.jpg"), ("2014", "train2014", "COCO_train2014_%012d.jpg"),
                                             ("2014_30k", "train2014", "COCO_train2014_%012d.jpg")])
def test_coco_paths_and_years(tmp_path, year, split, name):
    from pdm.utils.data import get_dataset
    base = F.write_coco(str(tmp_path), year, n=3)
    ds = get_dataset({"data_dir": base, "year": year})
    assert ds["validation"] is None                     # no captions_val file in the fixture
    tr = ds["train"]
    assert tr.column_names == ["image", "caption"] and len(tr) == 6           # one row per caption annotation
    assert tr[0]["image"] == os.path.join(base, "images", split, name % 1) and tr[1]["image"] == tr[0]["image"]
    assert tr[5]["caption"] == "the other caption and 2"
    assert all(os.path.exists(p) for p in tr["image"])


def test_caption_choice():
    from pdm.utils.data import pick_caption
    rng = np.random.default_rng(0)
    caps = ["a", "b", "c", "d"]
    assert pick_caption("x", True, rng) == "x" and pick_caption(caps, False, rng) == "a"
    got = {pick_caption(caps, True, rng) for _ in range(64)}
    assert got == set(caps)                             # training draws any of them
    with pytest.raises(ValueError):
        pick_caption(3, True, rng)


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("n", [16, 19])
def test_rank_shards_are_disjoint_and_cover(world, n):
    rows = [{"image": None, "caption": ""}] * n
    shards = [_loader(rows, rank=r, world=world, batch_size=3).epoch_indices(5) for r in range(world)]
    per = -(-n // world)
    assert all(len(s) == per for s in shards)
    assert len({len(_loader(rows, rank=r, world=world, batch_size=3)) for r in range(world)}) == 1    # same step count
    flat = [i for s in shards for i in s]
    assert set(flat) == set(range(n))                   # coverage
    if n % world == 0:
        assert len(flat) == len(set(flat))              # disjoint
    else:                                               # only the wrap-around padding repeats
        assert len(flat) - len(set(flat)) == per * world - n


def test_epoch_order_is_seeded():
    rows = [{"image": None, "caption": ""}] * 50
    a, b = _loader(rows, seed=7), _loader(rows, seed=7)
    assert a.epoch_indices(0) == b.epoch_indices(0) and a.epoch_indices(3) == b.epoch_indices(3)
    assert a.epoch_indices(0) != a.epoch_indices(1)
    assert _loader(rows, seed=8).epoch_indices(0) != a.epoch_indices(0)
    assert sorted(a.epoch_indices(2)) == list(range(50))
    assert _loader(rows, shuffle=False).epoch_indices(4) == list(range(50))


def test_max_samples_hub_ids_and_local_datasets(tmp_path):
    from datasets import load_from_disk
    from pdm.utils.data import get_dataset, limit, load_local_dataset
    base = F.write_coco(str(tmp_path), "2017", n=4)
    tr = get_dataset({"data_dir": base, "year": "2017"})["train"]
    assert len(limit(tr, 3)) == 3 and limit(tr, 3)["caption"] == tr["caption"][:3] and len(limit(tr, 100)) == 8
    assert limit(tr, None) is tr
    for name in ("rezashkv/controlled_distillation", "stabilityai/stable-diffusion-2-1"):
        with pytest.raises(FileNotFoundError):
            load_local_dataset(name)
        with pytest.raises(FileNotFoundError):
            get_dataset({"dataset_name": name})
    with pytest.raises(FileNotFoundError):
        get_dataset({"data_files": str(tmp_path / "missing.json")})
    # a local `datasets` directory without a validation split: the reference's split (test_size=0.083333, seed=42)
    path = F.write_style_dataset(str(tmp_path), n=24)
    ds = get_dataset({"dataset_name": path})
    want = load_from_disk(path).train_test_split(test_size=0.083333, seed=42)
    assert ds["train"]["prompt"] == want["train"]["prompt"] and ds["validation"]["prompt"] == want["test"]["prompt"]
    # data_files: a json-lines file read by the `json` builder
    jl = tmp_path / "rows.jsonl"
    jl.write_text("".join(f'{{"image": "x{i}.jpg", "caption": "c{i}"}}\n' for i in range(12)))
    ds = get_dataset({"data_files": str(jl)})
    assert len(ds["train"]) + len(ds["validation"]) == 12


def test_packed_batches_and_dropped_images(tmp_path):
    from PIL import Image
    from pdm.utils.data import DESC_BYTES, center_crop_origin, get_dataset, resized_size
    root = str(tmp_path)
    F.write_tokenizer(root)
    from pdm.utils.data import load_tokenizer, tokenize
    tok = load_tokenizer(root)
    base = F.write_coco(root, "2017", n=5, corrupt=(1, 3))
    tr = get_dataset({"data_dir": base, "year": "2017"})["train"]           # rows 2, 3, 6, 7 are the corrupt images
    ld = _loader(tr, tokenizer=tok, batch_size=3, shuffle=False, center_crop=True, train=False)
    batches = list(ld)
    assert len(batches) == len(ld) == 4 and ld.epoch == 1
    assert [b["index"].tolist() for b in batches] == [[0, 1], [4, 5], [8], [9]]
    ld.bs = 2
    empty = list(ld)[1]                                 # rows 2, 3: every image of the batch dropped
    assert empty["index"].numel() == 0 and empty["image_desc"].shape == (0, 8) and empty["input_ids"].shape == (0, F.T)
    b0 = batches[0]
    d = b0["image_desc"]
    head = 2 * DESC_BYTES
    assert torch.equal(b0["packed"][:head].view(torch.int64).view(2, 8), d)
    for k, i in enumerate(b0["index"].tolist()):
        a = np.asarray(Image.open(tr[i]["image"]).convert("RGB"))
        off, h, w, rh, rw, top, left, flip = d[k].tolist()
        assert (h, w) == a.shape[:2] and (rh, rw) == resized_size(h, w, 32) and (top, left) == center_crop_origin(rh, rw, 32)
        assert off % 4 == 0 and flip == 0
        assert np.array_equal(b0["packed"][head + off:head + off + a.size].numpy(), a.reshape(-1))
    # validation loader: the first caption of each row, tokenised with padding to model_max_length
    assert torch.equal(b0["input_ids"], tokenize(tok, [tr[i]["caption"] for i in b0["index"].tolist()]))
    assert torch.equal(b0["empty_input_ids"], tokenize(tok, [""] * 2))


def test_random_draws_do_not_depend_on_the_worker_count(tmp_path):
    from pdm.utils.data import get_dataset
    base = F.write_coco(str(tmp_path), "2017", n=8)
    tr = get_dataset({"data_dir": base, "year": "2017"})["train"]
    runs = []
    for nw in (0, 2):
        ld = _loader(tr, batch_size=3, num_workers=nw, seed=3, random_flip=True, rank=1, world=2)
        runs.append([(b["index"], b["image_desc"], b["captions"]) for _ in range(2) for b in ld])
    assert len(runs[0]) == len(runs[1]) == 6
    for (ia, da, ca), (ib, db, cb) in zip(*runs):
        assert torch.equal(ia, ib) and torch.equal(da, db) and ca == cb
    flips = torch.cat([d[:, 7] for _, d, _ in runs[0]])
    tops_lefts = torch.cat([d[:, 5:7] for _, d, _ in runs[0]])
    assert 0 < int(flips.sum()) < flips.numel()         # both flip outcomes are drawn
    assert int(tops_lefts.max()) > 0


def test_shared_packer_layout():
    """pack_images on images of 0, 1, 2 and 3 bytes mod 4: word-aligned offsets, zero gaps and spare word, the head equal to
    the descriptors; the CLIP and FID packers are this packer with their geometry."""
    from pdm.utils import clip_utils, fid_utils
    from pdm.utils.data import DESC_BYTES, center_crop_origin, pack_images, resized_size
    rng = np.random.default_rng(0)
    shapes = [(1, 1), (1, 3), (2, 3), (4, 4)]                                   # 3, 9, 18, 48 bytes
    arrays = [rng.integers(1, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    assert sorted(a.size % 4 for a in arrays) == [0, 1, 2, 3]
    rows = [[h, w, 10 + i, 20 + i, i, 2 * i, i % 2] for i, (h, w) in enumerate(shapes)]
    packed, desc = pack_images(arrays, rows)
    assert packed.dtype == torch.uint8 and desc.dtype == torch.int64 and tuple(desc.shape) == (4, 8)
    assert desc[:, 0].tolist() == [0, 4, 16, 36] and desc[:, 1:].tolist() == rows
    head = 4 * DESC_BYTES
    assert packed.numel() == head + 36 + 48 + 4
    buf = packed.numpy()
    assert buf[:head].view(np.int64).reshape(4, 8).tolist() == desc.tolist()
    used = np.zeros(buf.size, bool)
    used[:head] = True
    for o, a in zip(desc[:, 0].tolist(), arrays):
        assert o % 4 == 0 and np.array_equal(buf[head + o:head + o + a.size], a.reshape(-1))
        used[head + o:head + o + a.size] = True
    assert (~used).sum() == 1 + 3 + 2 + 0 + 4 and not buf[~used].any()         # the gaps and the spare word
    # a geometry callable gives the same rows
    same, d2 = pack_images(arrays, lambda h, w: (h + 1, w + 2, 3, 4, 1))
    assert d2[:, 1:].tolist() == [[h, w, h + 1, w + 2, 3, 4, 1] for h, w in shapes] and torch.equal(same[head:], packed[head:])
    # the named wrappers
    for R in (2, 5):
        want = pack_images(arrays, [[h, w, *resized_size(h, w, R), *center_crop_origin(*resized_size(h, w, R), R), 0] for h, w in shapes])
        got = clip_utils.pack_images(arrays, R)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    want = pack_images(arrays, [[h, w, h, w, 0, 0, 0] for h, w in shapes])
    got = fid_utils.pack_images(arrays)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # no images: descriptors [0, 8] and the spare word alone; anything but uint8 [H, W, 3] is refused
    packed, desc = pack_images([], [])
    assert tuple(desc.shape) == (0, 8) and packed.tolist() == [0, 0, 0, 0]
    for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2, 4), np.uint8), np.zeros((2, 2, 3), np.float32)):
        with pytest.raises(ValueError):
            pack_images([bad], lambda h, w: (h, w, 0, 0, 0))
