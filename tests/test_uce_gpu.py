"""UCE on the GPU (-m gpu): pdmk_spd_system_f64, pdmk_spd_factor_f64, pdmk_spd_solve_f64 and pdmk_uce_delta against the
oracles and bounds of tests/uce_fixtures.py, `edit_model` on the tiny topology against the fp64 restatement of the reference's
mat1 inverse(mat2), and train_erase.py + artist_erasure.py's loader on a tiny snapshot directory.

Bounds.  Factor and solve: the componentwise bounds of Higham's Thm 10.3 / 10.4 with gamma_{n+1} / gamma_{3n+1}, derived, not
measured.  System: the exact value is two roundings away, 2 ulp are allowed.  Delta: 4 x d_ref, d_ref = the distance of the
fp32 torch restatement of the reference's lines from the fp64 one.  The edit: 1 x d_ref of the fp32 restatement of
mat1 inverse(mat2), and the edit moves the weights by at least 100 x that bound."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import data_fixtures
import uce_fixtures as fx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---------------------------------------------------------------------------------------------- pdmk_spd_system_f64
def _gram(k, x, dev):
    n = x.shape[1]
    g = torch.zeros((n, n), device=dev, dtype=torch.float64)
    k.fid_accumulate(x.to(dev), torch.zeros(n, device=dev, dtype=torch.float64), g)
    return g


@pytest.mark.parametrize("with_b", [False, True], ids=["g_b_null", "g_b"])
@pytest.mark.parametrize("n", fx.SYSTEM_N)
def test_spd_system(dev, n, with_b):
    from pdm import _pdmk as k
    g = torch.Generator().manual_seed(n)
    xa, xb = torch.rand(37, n, generator=g), torch.rand(19, n, generator=g)          # non-negative: no cancellation in the sum
    ga, gb = _gram(k, xa, dev), (_gram(k, xb, dev) if with_b else None)
    lam, sa, sb = 0.5, 1.0 / 3.0, 0.1
    lda = n + 3
    A = torch.full((n, lda), NAN, device=dev, dtype=torch.float64)
    k.spd_system(ga, sa, gb, sb, lam, A[:, :n])
    A = A.cpu()
    assert bool(torch.isnan(A[:, n:]).all())
    Ga = fx.mirror_gram(ga.cpu())
    assert torch.equal(Ga, Ga.T) and torch.allclose(Ga, xa.double().T @ xa.double(), rtol=1e-12, atol=0)
    want = np.longdouble(lam) * np.eye(n, dtype=np.longdouble) + np.longdouble(sa) * fx._ld(Ga)
    if with_b:
        want = want + np.longdouble(sb) * fx._ld(fx.mirror_gram(gb.cpu()))
    got = fx._ld(A[:, :n])
    ulps = np.abs(got - want) / np.spacing(np.abs(want).astype(np.float64))
    print(f"spd_system n = {n}: worst {float(ulps.max()):.2f} ulp")
    assert float(ulps.max()) <= 2.0


# ---------------------------------------------------------------------------------------------- pdmk_spd_factor_f64
def _factor(k, A, dev, pad=5):
    """(L with NaN padding columns as read back, info) of the kernel on a copy of A [n, n] inside an [n, n + pad] buffer."""
    n = A.shape[0]
    buf = torch.full((n, n + pad), NAN, device=dev, dtype=torch.float64)
    buf[:, :n] = A.to(dev)
    info = torch.zeros(1, device=dev, dtype=torch.int32)
    k.spd_factor(buf[:, :n], info)
    return buf, int(info.item())


_FACTORED = {}


def _factored(k, n, dev):
    """A, the device buffer that holds L, and the checks of the factorisation itself - once per n, shared with the solve tests."""
    if n not in _FACTORED:
        A = fx.spd_matrix(n, seed=n)
        buf, info = _factor(k, A, dev)
        _FACTORED[n] = (A, buf, info)
    return _FACTORED[n]


def _check_factor(k, n, dev):
    A, buf, info = _factored(k, n, dev)
    assert info == 0
    host = buf.cpu()
    assert bool(torch.isnan(host[:, n:]).all()) and torch.equal(_bits(host[:, n:]), _bits(torch.full_like(host[:, n:], NAN)))
    L = torch.tril(host[:, :n])
    assert not bool(torch.isnan(L).any()) and bool((torch.diagonal(L) > 0).all())
    ex = fx.factor_excess(A, L)
    print(f"spd_factor n = {n}: |A - L L^T| at {ex:.3f} of gamma_(n+1) |L||L|^T")
    assert ex <= 1.0
    again, info2 = _factor(k, A, dev)
    assert info2 == 0 and torch.equal(_bits(torch.tril(again[:, :n]).cpu()), _bits(L))        # the same bits from a second run


@pytest.mark.parametrize("n", fx.FACTOR_N + [1024])
def test_spd_factor(dev, n):
    from pdm import _pdmk as k
    _check_factor(k, n, dev)


@pytest.mark.parametrize("n,col", [(40, 0), (130, 70)])
def test_spd_factor_not_positive_definite(dev, n, col):
    from pdm import _pdmk as k
    A = fx.spd_matrix(n, seed=3)
    L = torch.linalg.cholesky(A)
    # the pivot of column `col` is A[col, col] - sum_{q < col} L[col, q]^2: lower the diagonal entry by twice the pivot
    A[col, col] -= 2 * float(L[col, col]) ** 2
    buf, info = _factor(k, A, dev)
    assert info == col + 1                                            # and the call returned
    assert bool(torch.isnan(buf[:, n:]).all())
    head = torch.tril(buf[:col, :col]).cpu()
    # the columns before it are the factor's: two backward-stable factorisations differ by about cond(A) n u = 1e6 * 130 * 1e-16
    assert col == 0 or float((head - L[:col, :col]).abs().max()) <= 1e-7 * float(L.abs().max())


def test_spd_rejects(dev):
    from pdm import _pdmk as k
    A = torch.eye(8, device=dev, dtype=torch.float64)
    info = torch.zeros(1, device=dev, dtype=torch.int32)
    with pytest.raises(k.PdmkError):
        k.spd_factor(A.float(), info)
    with pytest.raises(k.PdmkError):
        k.spd_factor(A.t()[:, ::2], info)
    with pytest.raises(k.PdmkError):
        k.spd_solve(A, torch.zeros(3, 9, device=dev), torch.zeros(3, 9, device=dev))
    assert k._lib.pdmk_spd_factor_f64(A.data_ptr(), 5000, 5000, info.data_ptr(), None) == -1
    assert k._lib.pdmk_spd_solve_f64(A.data_ptr(), 8, 8, A.data_ptr(), 3, 8, A.data_ptr(), 8, None, 0, A.data_ptr(), 1, None) == -1
    assert k._lib.pdmk_spd_workspace_elems(130, 77) >= 77 * 130


# ---------------------------------------------------------------------------------------------- pdmk_spd_solve_f64
def _solve(k, Lbuf, n, B, dev, pad=3):
    """(X fp32, X64) of the kernel; B, X and X64 are column slices of wider buffers whose padding holds NaN."""
    m = B.shape[0]
    bb = torch.full((m, n + pad), NAN, device=dev)
    bb[:, :n] = B.to(dev)
    xb = torch.full((m, n + pad + 1), NAN, device=dev)
    x64 = torch.full((m, n + pad + 2), NAN, device=dev, dtype=torch.float64)
    k.spd_solve(Lbuf[:, :n], bb[:, :n], xb[:, :n], x64[:, :n])
    assert bool(torch.isnan(xb[:, n:]).all()) and bool(torch.isnan(x64[:, n:]).all())
    return xb[:, :n].cpu(), x64[:, :n].cpu()


def _check_solve(k, n, m, dev):
    A, buf, info = _factored(k, n, dev)
    assert info == 0
    B = fx.rhs(m, n, seed=100 + m)
    X, X64 = _solve(k, buf, n, B, dev)
    assert not bool(torch.isnan(X64).any())
    assert torch.equal(_bits(X), _bits(X64.float()))
    ex = fx.solve_excess(A, buf[:, :n].cpu(), B, X64)
    print(f"spd_solve n = {n}, m = {m}: |B - X A| at {ex:.4f} of gamma_(3n+1) |X| |L||L|^T")
    assert ex <= 1.0
    return B, X, X64


@pytest.mark.parametrize("m", fx.SOLVE_M)
@pytest.mark.parametrize("n", fx.FACTOR_N)
def test_spd_solve(dev, n, m):
    from pdm import _pdmk as k
    _check_solve(k, n, m, dev)


def test_spd_solve_1024_and_row_blocks_are_independent(dev):
    from pdm import _pdmk as k
    n = 1024
    B, X, X64 = _check_solve(k, n, 154, dev)
    _A, buf, _info = _factored(k, n, dev)
    for half in (slice(0, 77), slice(77, 154)):
        Xh, X64h = _solve(k, buf, n, B[half], dev)
        assert torch.equal(_bits(X64h), _bits(X64[half])) and torch.equal(_bits(Xh), _bits(X[half]))
    # without the optional fp64 output
    x = torch.empty((154, n), device=dev)
    k.spd_solve(buf[:, :n], B.to(dev), x)
    assert torch.equal(_bits(x.cpu()), _bits(X))


def test_spd_solve_small_row_blocks_are_independent(dev):
    from pdm import _pdmk as k
    n = 130
    B, X, X64 = _check_solve(k, n, 154, dev)
    _A, buf, _info = _factored(k, n, dev)
    for half in (slice(0, 77), slice(77, 154)):
        _Xh, X64h = _solve(k, buf, n, B[half], dev)
        assert torch.equal(_bits(X64h), _bits(X64[half]))


# ---------------------------------------------------------------------------------------------- pdmk_uce_delta
@pytest.mark.parametrize("technique", ["replace", "tensor"])
@pytest.mark.parametrize("Q", [1, 4])
@pytest.mark.parametrize("P", [1, 3])
def test_uce_delta(dev, P, Q, technique):
    from pdm import _pdmk as k
    from pdm.utils.uce import TECHNIQUES
    row_seg = [0, 11] if P == 1 else [0, 1, 12, 19]                   # a 1-row pair
    col_seg = [0, 72] if Q == 1 else [0, 64, 72, 200, 264]
    m, w, ld = 24, col_seg[-1], col_seg[-1] + 8
    g = torch.Generator().manual_seed(7 * P + Q)
    O, N = torch.randn(m, w, generator=g), torch.randn(m, w, generator=g)
    N = N + 0.7 * O                                                   # a projection of N on O that matters
    zero_block = P == 3 and Q == 4
    if zero_block:
        O[row_seg[1]:row_seg[2], col_seg[2]:col_seg[3]] = 0
    bufs = [torch.full((m, ld), 1e4, device=dev) for _ in range(3)]
    bufs[0][:, :w], bufs[1][:, :w] = O.to(dev), N.to(dev)
    k.uce_delta(bufs[0][:, :w], bufs[1][:, :w], bufs[2][:, :w], row_seg, col_seg, TECHNIQUES.index(technique))
    out = bufs[2].cpu()
    assert bool((out[:, w:] == 1e4).all())                            # the padding columns are untouched
    D = out[:, :w]
    assert bool((D[row_seg[-1]:] == 0).all())                         # the padding rows are zeroed
    ref64 = fx.reference_delta(O, N, row_seg, col_seg, technique, torch.float64)
    ref32 = fx.reference_delta(O, N, row_seg, col_seg, technique, torch.float32)
    d_ref, d = fx.distance([ref32], [ref64]), fx.distance([D], [ref64])
    print(f"uce_delta P = {P}, Q = {Q}, {technique}: d_ref {d_ref:.3e}, kernel {d:.3e}")
    assert d <= 4 * d_ref
    if zero_block:
        blk = (slice(row_seg[1], row_seg[2]), slice(col_seg[2], col_seg[3]))
        assert torch.equal(D[blk], N[blk])
    again = torch.empty_like(bufs[2])
    k.uce_delta(bufs[0][:, :w], bufs[1][:, :w], again[:, :w], row_seg, col_seg, TECHNIQUES.index(technique))
    assert torch.equal(_bits(again[:, :w].cpu()), _bits(D))


# ---------------------------------------------------------------------------------------------- the edit, tiny topology
def _script(name, sub):
    spec = importlib.util.spec_from_file_location(name + "_uce_gpu", os.path.join(ROOT, "unlearn-ft_amd", "scripts", sub, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tree(tmp_path_factory, dev):
    """data_fixtures.write_pruned_checkpoint_tree plus the script's config and the frozen models over it."""
    from pdm.utils.load_models import FrozenModels, inference_config
    t = data_fixtures.write_pruned_checkpoint_tree(str(tmp_path_factory.mktemp("uce")), dev, "uce.yaml")
    config = inference_config(t["yaml"], t["snap"], tiny=True)
    models = FrozenModels(config, dev)
    return dict(t, config=config, models=models, tokenizer=models.tokenizer)


def _load(tree):
    return tree["models"].load_unet(tree["ck"])


def _is_kv(name):
    return name.endswith(".attn2.to_k.weight") or name.endswith(".attn2.to_v.weight")


def _embeddings(tree, groups, dev):
    """{text: (fp32 [T, K] on the CPU, attention-mask sum)}; every group of texts is one call of the text encoder, as in the
    edit (the same batch shapes: the same kernels, the same bits)."""
    out = {}
    for texts in groups:
        if not texts:
            continue
        tok = tree["tokenizer"](texts, padding="max_length", max_length=tree["tokenizer"].model_max_length, truncation=True,
                                return_tensors="pt")
        emb = tree["models"].text_encoder(tok.input_ids.to(dev))[0].float().cpu()
        out.update({t: (emb[i], int(tok.attention_mask[i].sum())) for i, t in enumerate(texts)})
    return out


def _sample(tree, unet, dev):
    from pdm.pipelines.pruning_pipelines import PNDMScheduler, StableDiffusionPruningPipeline
    pipe = StableDiffusionPruningPipeline(tree["models"].vae, None, unet, PNDMScheduler(prediction_type="v_prediction"))
    g = torch.Generator().manual_seed(4)
    pe, ne, lat = (torch.randn(1, data_fixtures.T, 64, generator=g), torch.randn(1, data_fixtures.T, 64, generator=g),
                   torch.randn(1, 4, 16, 16, generator=g))
    return pipe(prompt_embeds=pe.to(dev), negative_prompt_embeds=ne.to(dev), latents=lat.to(dev), num_inference_steps=3,
                guidance_scale=7.5, output_type="latent").images.cpu()


EDIT_CASES = {
    # name: (old texts, new texts, retain texts or None, technique)
    "replace_retain": (["van gogh"], ["art"], ["", "monet", "the sea and the sky"], "replace"),
    "tensor_retain": (["van gogh"], ["art"], ["", "monet", "the sea and the sky"], "tensor"),
    "replace_only_empty": (["van gogh"], [""], None, "replace"),
    "tensor_two_concepts": (["van gogh", "style of the monet"], ["a painter", "art"], [""], "tensor"),
}


@pytest.mark.parametrize("case", list(EDIT_CASES))
def test_edit_model(dev, tree, case, tmp_path):
    from pdm.utils import uce as U
    old, new, retain, technique = EDIT_CASES[case]
    lamb, s_e = U.LAMB, 1.0
    ret = [""] if retain is None else retain
    s_r = U.default_preserve_scale(None, ret)
    unet = _load(tree)
    before = _sample(tree, unet, dev) if case == "replace_retain" else None
    U.edit_model(unet, tree["models"].text_encoder, tree["tokenizer"], old, new, retain, lamb=lamb, erase_scale=s_e,
                 preserve_scale=s_r, technique=technique)
    sd = unet.state_dict()
    assert list(sd) == list(tree["sd"])
    kv = [n for n in sd if _is_kv(n)]
    assert len(kv) >= 4
    for n, v in sd.items():
        if _is_kv(n):
            assert v.dtype == torch.float32 and not torch.equal(v, tree["sd"][n]), n         # every one of them changed
        else:
            assert v.dtype == tree["sd"][n].dtype and torch.equal(v, tree["sd"][n]), n

    new_ = [" " if t == "" else t for t in new]
    erase = list(dict.fromkeys(old + new_))
    E = _embeddings(tree, [erase, [t for t in dict.fromkeys(ret) if t not in erase]], dev)
    T = data_fixtures.T
    pairs = []
    for o, n in zip(old, new_):
        so, sn = fx.slices(E[o][1], E[n][1], T)
        pairs.append((E[o][0][so], E[n][0][sn]))
        assert pairs[-1][0].shape == pairs[-1][1].shape and pairs[-1][0].shape[0] >= 2
    if case == "tensor_two_concepts":
        assert len({E[t][1] for t in old + new_}) >= 3                # guiding texts of other token lengths than the concepts
    rets = [E[t][0] for t in ret]
    ref64 = [fx.reference_edit(tree["sd"][n], pairs, rets, lamb, s_e, s_r, technique, torch.float64) for n in kv]
    ref32 = [fx.reference_edit(tree["sd"][n], pairs, rets, lamb, s_e, s_r, technique, torch.float32) for n in kv]
    d_ref = fx.distance(ref32, ref64)
    d = fx.distance([sd[n] for n in kv], ref64)
    moved = fx.distance([tree["sd"][n] for n in kv], ref64)
    print(f"edit {case}: d_ref {d_ref:.3e}, edit {d:.3e}, moved {moved:.3e}")
    assert moved >= 100 * d_ref                                       # the check is not empty
    assert d <= d_ref

    if case == "replace_retain":
        # the compute copies were refreshed: the sampler sees the edit, and a model loaded from the saved file samples the same bits
        after = _sample(tree, unet, dev)
        assert not torch.equal(after, before)
        path = str(tmp_path / "erased.pt")
        torch.save(sd, path)
        other = _load(tree)
        other.load_state_dict(torch.load(path, map_location="cpu"))
        assert torch.equal(_bits(_sample(tree, other, dev)), _bits(after))


def test_edit_model_raises_when_not_positive_definite(dev, tree):
    from pdm.utils import uce as U
    unet = _load(tree)
    with pytest.raises(RuntimeError, match="not positive definite at column 0"):
        U.edit_model(unet, tree["models"].text_encoder, tree["tokenizer"], ["van gogh"], ["art"], [""], lamb=-1e6)
    assert all(torch.equal(v, tree["sd"][n]) for n, v in unet.state_dict().items())           # no weight was touched


def test_script_on_a_tiny_snapshot(dev, tree):
    from pdm.utils import erasure_utils as E
    out_dir = os.path.join(tree["root"], "out")
    script = _script("train_erase", "baselines/unified_concept_editing")
    # --guided_concept: the spelling of the reference's run.sh (argparse's prefix matching)
    ckpt = script.main(["--concepts", "Van Gogh", "--guided_concept", "art", "--concept_type", "art", "--base_config_path",
                        tree["yaml"], "--model_id", tree["snap"], "--ckpt_path", tree["ck"] + "/", "--output_dir", out_dir,
                        "--preserve_number", "5", "--tiny"])
    name = "erased-van gogh-towards_art-preserving_5artists-preserve_true-sd_2_1-method_replace"
    assert ckpt == os.path.join(out_dir, "models", name + ".pt") and os.path.exists(ckpt)
    with open(os.path.join(out_dir, "info", name + ".txt")) as f:
        assert json.load(f) == ["Van Gogh"]
    sd = torch.load(ckpt, map_location="cpu")
    assert list(sd) == list(tree["sd"]) and all(v.dtype == tree["sd"][n].dtype for n, v in sd.items())
    assert all(torch.equal(v, tree["sd"][n]) != _is_kv(n) for n, v in sd.items())
    E.check_baseline("uce", ckpt_name=ckpt)
    erasure = _script("artist_erasure", "metrics")
    a = erasure.parse_args(["--target", "Van Gogh", "--baseline", "uce", "--base_config_path", tree["yaml"], "--model_id",
                            tree["snap"], "--original_ckpt", tree["ck"] + "/", "--ckpt_name", ckpt, "--tiny"])
    original, erased = E.load_pipelines(tree["config"], a, dev)
    got = erased.unet.state_dict()
    assert all(torch.equal(got[n], v) for n, v in sd.items())
    assert all(torch.equal(v, tree["sd"][n]) for n, v in original.unet.state_dict().items())
