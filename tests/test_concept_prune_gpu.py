"""ConceptPrune on the GPU (-m gpu): pdmk_rownorm_colsq, pdmk_wanda_count and pdmk_wanda_apply against the CPU oracles of
tests/concept_prune_fixtures.py, the WandaObserver inside the sampler on the tiny topology, and wanda.py +
save_union_over_time.py + artist_erasure.py's loader on a tiny snapshot directory.

Tolerance of the observation: the kernel sums in another order than torch, and that earns what the reference's own fp32
arithmetic is away from fp64 and no more - in each test d_ref, the largest relative distance of the fp32 CPU restatement
(chained sqrt(old^2 + new^2) over the same calls) from the fp64 one, is computed and the kernel may be 4 x d_ref away.
Scores and masks are compared exactly."""
import importlib.util
import os

import pytest
import torch

import concept_prune_fixtures as fx
import data_fixtures

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16]


def _ids(v):
    return "x".join(str(a) for a in v) if isinstance(v, tuple) else str(v).replace("torch.", "")


# ---------------------------------------------------------------------------------------------- pdmk_rownorm_colsq
def _observe(k, xs, dev, dtype, pad=0):
    """sqrt (in fp64) of the accumulator after one call per x; pad: columns of 1e4 behind every row that must not be read."""
    Fd = xs[0].shape[1]
    acc = torch.zeros(Fd, device=dev)
    for x in xs:
        buf = torch.full((x.shape[0], Fd + pad), 1e4, device=dev, dtype=dtype)
        buf[:, :Fd] = x.to(dev, dtype)
        k.rownorm_colsq(buf[:, :Fd], acc)
    return acc.cpu()


def _check_colnorm(k, xs, dev, dtype, pad=0, what=""):
    acc = _observe(k, xs, dev, dtype, pad)
    assert not torch.isnan(acc).any() and bool((acc >= 0).all())
    ref64 = fx.colnorm_oracle(xs, torch.float64)
    d_ref = fx.rel_distance(fx.colnorm_oracle(xs, torch.float32), ref64)
    d = fx.rel_distance(acc.double().sqrt(), ref64)
    print(f"rownorm_colsq {what}: d_ref {d_ref:.3e}, kernel {d:.3e}")
    assert d <= 4 * d_ref, (d, d_ref)
    return acc


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", fx.ROWNORM_SHAPES, ids=_ids)
def test_rownorm_colsq(dev, shape, dtype):
    from pdm import _pdmk as k
    M, Fd = shape
    x = fx.activations(M, Fd, seed=1)
    acc = _check_colnorm(k, [x], dev, dtype, what=f"{M}x{Fd} {_ids(dtype)}")
    again = _observe(k, [x], dev, dtype)
    assert torch.equal(acc, again)                                   # bit-equal from launch to launch
    # the row normalisation is there: every row adds at most 1 in total, whatever its scale
    nonzero_rows = int((x.abs().sum(1) > 0).sum())
    assert abs(float(acc.double().sum()) - nonzero_rows) <= 1e-4 * max(nonzero_rows, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_rownorm_colsq_accumulates_and_skips_padding(dev, dtype):
    from pdm import _pdmk as k
    xs = [fx.activations(384, 72, seed=10 + i) for i in range(5)]
    _check_colnorm(k, xs, dev, dtype, what=f"384x72 x 5 calls {_ids(dtype)}")
    xs = [fx.activations(130, 72, seed=3), fx.activations(63, 72, seed=4)]
    a = _check_colnorm(k, xs, dev, dtype, pad=24, what=f"130x72 + 63x72, ld = 96, {_ids(dtype)}")
    assert torch.equal(a, _observe(k, xs, dev, dtype, pad=0))        # the padding columns were not read


def test_rownorm_colsq_rejects(dev):
    from pdm import _pdmk as k
    acc = torch.zeros(80, device=dev)
    with pytest.raises(k.PdmkError):
        k.rownorm_colsq(torch.zeros(4, 12, device=dev), acc)           # F % 8
    with pytest.raises(k.PdmkError):
        k.rownorm_colsq(torch.zeros(4, 16, device=dev), acc[:8])       # accumulator shorter than F


# ---------------------------------------------------------------------------------------------- pdmk_wanda_count
def _count(k, w, nb, nt, kk, dev, dtype, pad=0, start=None):
    O, Fd = w.shape
    buf = torch.full((O, Fd + pad), 1e4, device=dev, dtype=dtype)
    buf[:, :Fd] = w.to(dev, dtype)
    count = torch.zeros((O, Fd), device=dev, dtype=torch.int32) if start is None else start.to(dev).clone()
    k.wanda_count(buf[:, :Fd], nb.to(dev), nt.to(dev), kk, count)
    return count.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", fx.COUNT_CASES, ids=_ids)
def test_wanda_count(dev, case, dtype):
    from pdm import _pdmk as k
    from pdm.utils.concept_prune import top_k
    O, Fd, T, ratio = case
    w, nb, nt = fx.count_inputs(O, Fd, T)
    w = w.to(dtype).to(torch.float32)
    kk = top_k(ratio, Fd)
    ref = fx.count_oracle(w, nb, nt, kk, check_no_tie=True)
    got = _count(k, w, nb, nt, kk, dev, dtype)
    assert got.dtype == torch.int32 and torch.equal(got, ref), int((got != ref).sum())
    if kk == 0:
        assert int(got.abs().sum()) == 0
    else:
        dens = float((ref > 0).float().mean())
        print(f"wanda_count {case}: k = {kk}, density of count > 0: {dens:.3f}")
        assert dens > 0.01
    # accumulated into, and the same bits from a second launch
    start = torch.arange(O * Fd, dtype=torch.int32).reshape(O, Fd) % 7
    assert torch.equal(_count(k, w, nb, nt, kk, dev, dtype, start=start), ref + start)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_wanda_count_row_stride(dev, dtype):
    from pdm import _pdmk as k
    w, nb, nt = fx.count_inputs(40, 200, 3)
    w = w.to(dtype).to(torch.float32)
    assert torch.equal(_count(k, w, nb, nt, 20, dev, dtype, pad=24), fx.count_oracle(w, nb, nt, 20))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_wanda_count_ties_zero_rows_and_equal_norms(dev, dtype):
    from pdm import _pdmk as k
    O, Fd, T, kk = 40, 200, 2, 20
    w, nb, nt = fx.tie_inputs(O, Fd, T, kk, dtype)
    assert fx.straddling_ties(w, nt, kk) >= O                         # the tie group lies across the k-th place
    ref = fx.count_oracle(w, nb, nt, kk)
    got = _count(k, w, nb, nt, kk, dev, dtype)
    assert torch.equal(got, ref), int((got != ref).sum())
    assert int(ref[1].sum()) <= 3 * T and int((ref[1] > 0).sum()) <= 3        # the row with three non-zero weights
    same = torch.arange(8) * (Fd // 8) + 11
    assert int(got[:, same].sum()) == 0                               # n_target == n_base: strictly greater, not counted


def test_wanda_count_too_wide_raises(dev):
    from pdm import _pdmk as k
    w = torch.zeros(2, 8200, device=dev)
    n = torch.ones(1, 8200, device=dev)
    with pytest.raises(k.PdmkError):
        k.wanda_count(w, n, n, 10, torch.zeros(2, 8200, device=dev, dtype=torch.int32))
    # the library's own status, not only the wrapper's check
    rc = k._lib.pdmk_wanda_count(w.data_ptr(), k.F32, 2, 8200, 8200, n.data_ptr(), n.data_ptr(), 1, 10,
                                 torch.zeros(2, 8200, device=dev, dtype=torch.int32).data_ptr(), None)
    assert rc == -2


# ---------------------------------------------------------------------------------------------- pdmk_wanda_apply
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("half", [False, True], ids=["thr0", "thr_half"])
def test_wanda_apply(dev, dtype, half):
    from pdm import _pdmk as k
    from pdm.utils.concept_prune import count_threshold
    O, Fd, T, off, wide = 37, 72, 6, 8, 96
    g = torch.Generator().manual_seed(5)
    count = torch.tensor([0, 1, T], dtype=torch.int32)[torch.randint(0, 3, (O, Fd), generator=g)]
    full = (torch.randn(O, wide, generator=g) + 3).to(dtype)
    buf = full.to(dev).clone()
    thr = count_threshold(0.5 if half else 0.0, T)
    k.wanda_apply(buf[:, off:off + Fd], count.to(dev), thr)
    want = full.clone()
    want[:, off:off + Fd][count.to(torch.float32) > thr] = 0
    assert torch.equal(buf.cpu(), want)                               # masked entries zero, neighbours and the rest untouched
    assert int((want[:, off:off + Fd] == 0).sum()) == int((count > (T // 2 if half else 0)).sum())


# ---------------------------------------------------------------------------------------------- observer in the sampler
def _pipe(dev, dtype, scheduler):
    from pdm_ref import arch as oarch, weights as oweights, vae as ovae
    from pdm_ref.config import UNetConfig as OCfg
    from pdm.models.unet.spec import UNetConfig
    from pdm.models.unet.unet_2d_conditional import UNet2DConditionModelPruned
    from pdm.models.vae.autoencoder_kl import AutoencoderKL, VAEConfig
    from pdm.pipelines.pruning_pipelines import StableDiffusionPruningPipeline
    ocfg, cfg = OCfg.tiny(), UNetConfig.tiny()
    dense = oweights.init_dense_state_dict(ocfg, seed=0)
    av = oarch.random_arch_vector(ocfg, 0.6, seed=1, drop_depth=(1,))
    unet = UNet2DConditionModelPruned(cfg, av, dev, dtype, train=False, init=False)
    unet.load_dense_or_pruned(dense)
    vcfg = ovae.VAEConfig.tiny()
    vae = AutoencoderKL(VAEConfig(block_out_channels=vcfg.block_out_channels, layers_per_block=1), dev, dtype, init=False)
    vae.load_state_dict(ovae.init_state_dict(vcfg, seed=7))
    return StableDiffusionPruningPipeline(vae, None, unet, scheduler)


class _Capture:
    """An observer that keeps a host copy of every tensor it is handed, in call order."""

    def __init__(self):
        self.calls = []

    def __call__(self, layer, gl):
        self.calls.append((layer, gl.to(torch.float32).cpu()))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_observer_in_the_sampler(dev, dtype):
    from pdm.pipelines.pruning_pipelines import DDIMScheduler
    from pdm.utils import concept_prune as CP
    steps = 3
    pipe = _pipe(dev, dtype, DDIMScheduler(prediction_type="v_prediction"))
    unet = pipe.unet
    g = torch.Generator().manual_seed(4)
    prompts = [torch.randn(1, 13, 64, generator=g) for _ in range(2)]
    neg = torch.randn(1, 13, 64, generator=g)
    lat = torch.randn(1, 4, 16, 16, generator=g)

    def run(i):
        return pipe(prompt_embeds=prompts[i], negative_prompt_embeds=neg, latents=lat, num_inference_steps=steps,
                    guidance_scale=7.5, output_type="latent").images

    plain = [run(i) for i in range(2)]                               # no observer
    obs = CP.WandaObserver(unet, steps)
    layers = CP.ffn_layers(unet)
    L = len(layers)
    assert L >= 2 and [key for key, *_ in layers] == sorted(key for key, *_ in layers)
    assert [key + ".weight" for key, *_ in layers] == [n for n in unet.state_dict() if n.endswith("ff.net.2.weight")]
    seen = []
    for i in range(2):
        obs.reset_time_layer()
        with CP.observing(unet, obs):
            assert pipe._use_graph(None, None) is False               # an observer selects the eager loop
            seen.append(run(i))
        assert (obs.call, obs.layer) == (steps, 0)
    assert unet.engine.ffn_observer is None
    cap = _Capture()
    for i in range(2):
        with CP.observing(unet, cap):
            again = run(i)
        assert torch.equal(again, seen[i]) and torch.equal(again, plain[i])     # observing changes nothing that is computed
    # the arena rebuilt on the host from the captured tensors: slot (t, l), both CFG halves, both prompts
    assert len(cap.calls) == 2 * steps * L and [l for l, _ in cap.calls] == list(range(L)) * (2 * steps)
    got = obs.norms()
    worst = (0.0, 0.0)
    for l, (key, O, Fd, Fp) in enumerate(layers):
        assert got[l].shape == (steps, Fd)
        for t in range(steps):
            xs = [cap.calls[(i * steps + t) * L + l][1] for i in range(2)]
            assert all(x.shape[1] == Fp and x.shape[0] % 2 == 0 for x in xs), key         # both CFG halves
            assert all(bool((x[:, Fd:] == 0).all()) for x in xs)                   # padding columns carry nothing
            xs = [x[:, :Fd] for x in xs]
            ref64 = fx.colnorm_oracle(xs, torch.float64)
            d_ref = fx.rel_distance(fx.colnorm_oracle(xs, torch.float32), ref64)
            acc = obs.arena.view(steps, obs.width)[t, obs.offsets[l]:obs.offsets[l] + Fd].cpu()
            d = fx.rel_distance(acc.double().sqrt(), ref64)
            assert d <= 4 * d_ref, (key, t, d, d_ref)
            if d > worst[0]:
                worst = (d, d_ref)
    print(f"observer {_ids(dtype)}: worst kernel distance {worst[0]:.3e} (d_ref there {worst[1]:.3e})")
    # reset_time_layer() is what starts a run: without it the next call has no slot
    with CP.observing(unet, obs):
        with pytest.raises(RuntimeError, match="timestep slots"):
            run(0)


def test_observer_pndm_repeats_slot_zero(dev):
    from pdm.pipelines.pruning_pipelines import PNDMScheduler
    from pdm.utils import concept_prune as CP
    steps = 3
    pipe = _pipe(dev, torch.float32, PNDMScheduler(prediction_type="epsilon"))
    g = torch.Generator().manual_seed(4)
    pe, ne, lat = torch.randn(1, 13, 64, generator=g), torch.randn(1, 13, 64, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    obs = CP.WandaObserver(pipe.unet, steps, repeat_first=True)
    cap = _Capture()
    for o in (obs, cap):
        with CP.observing(pipe.unet, o):
            pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=steps, output_type="latent")
    L = obs.L
    assert obs.call == steps + 1 and len(cap.calls) == (steps + 1) * L
    Fd = obs.layers[0][2]
    for t, calls in enumerate([(0, 1), (2,), (3,)]):
        xs = [cap.calls[c * L][1][:, :Fd] for c in calls]
        ref64 = fx.colnorm_oracle(xs, torch.float64)
        d_ref = fx.rel_distance(fx.colnorm_oracle(xs, torch.float32), ref64)
        acc = obs.arena.view(steps, obs.width)[t, :Fd].cpu()
        assert fx.rel_distance(acc.double().sqrt(), ref64) <= 4 * d_ref


# ---------------------------------------------------------------------------------------------- the scripts, tiny snapshot
def _script(name, sub="baselines/concept_prune"):
    spec = importlib.util.spec_from_file_location(name + "_cp_gpu", os.path.join(ROOT, "unlearn-ft_amd", "scripts", sub, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tree(tmp_path_factory, dev):
    """data_fixtures.write_pruned_checkpoint_tree plus a two-word list."""
    t = data_fixtures.write_pruned_checkpoint_tree(str(tmp_path_factory.mktemp("concept_prune")), dev, "cp.yaml")
    words = os.path.join(t["root"], "words")
    os.makedirs(words)
    with open(os.path.join(words, "things.txt"), "w") as f:
        f.write("cat\ndog\n")
    return dict(t, words=words)


def test_scripts_on_a_tiny_snapshot(dev, tree):
    from pdm.utils import concept_prune as CP, erasure_utils as E
    T, ratio = 3, 0.25
    argv = ["--target", "Monet", "--base_config_path", tree["yaml"], "--model_id", tree["snap"], "--ckpt_path", tree["ck"] + "/",
            "--result_dir", os.path.join(tree["root"], "res"), "--words_dir", tree["words"], "--timesteps", str(T),
            "--skill_ratio", str(ratio), "--image_resolution", "64", "--tiny", "--seed", "0"]
    wanda, union = _script("wanda"), _script("save_union_over_time")
    counts_file = wanda.main(argv)
    res = os.path.join(tree["root"], "res", "snapshot", "Monet")
    assert counts_file == os.path.join(res, "skilled_neurons", str(ratio), "union_counts.pt")
    assert sorted(os.listdir(os.path.join(res, "images"))) == sorted(f"{n}_{i}.jpg" for n in ("base", "target") for i in range(2))
    base, target = (CP.load_norms(os.path.join(res, n)) for n in ("base_norms.pt", "target_norms.pt"))
    raw = torch.load(os.path.join(res, "base_norms.pt"))
    assert sorted(raw) == list(range(T)) and sorted(raw[0]) == list(range(len(base))) and raw[0][0].dim() == 1
    counts = torch.load(counts_file)
    names = [n for n in tree["sd"] if n.endswith("ff.net.2.weight")]
    assert [k + ".weight" for k in counts] == names
    oracle = {}
    for l, n in enumerate(names):
        w = tree["sd"][n]
        assert base[l].shape == (T, w.shape[1]) and not torch.equal(base[l], target[l])
        oracle[n] = fx.count_oracle(w, base[l], target[l], CP.top_k(ratio, w.shape[1]))
        assert counts[n[:-len(".weight")]].dtype == torch.int32 and torch.equal(counts[n[:-len(".weight")]], oracle[n]), n
    assert sum(int((c > 0).sum()) for c in oracle.values()) > 0
    # a second run reloads the norms: no sampling (the images keep their time stamps), the same counts
    stamp = {n: os.stat(os.path.join(res, "images", n)).st_mtime_ns for n in os.listdir(os.path.join(res, "images"))}
    wanda.main(argv)
    assert {n: os.stat(os.path.join(res, "images", n)).st_mtime_ns for n in stamp} == stamp
    assert all(torch.equal(v, counts[k]) for k, v in torch.load(counts_file).items())

    for select in (0.0, 0.5):
        ckpt = union.main(argv + ["--select_ratio", str(select)])
        assert ckpt == os.path.join(res, "checkpoints", f"skill_ratio_{ratio}_timesteps_{T}_threshold{select}.pt")
        sd = torch.load(ckpt)
        assert list(sd) == list(tree["sd"])
        masked_any = False
        for n, v in sd.items():
            if n in oracle:
                mask = oracle[n].to(torch.float32) > select * T
                masked_any |= bool(mask.any())
                assert v.dtype == torch.float16
                assert bool((v[mask] == 0).all())
                assert torch.equal(v[~mask], tree["sd"][n].to(torch.float16)[~mask]), n
            else:
                assert v.dtype == tree["sd"][n].dtype and torch.equal(v, tree["sd"][n]), n
        assert masked_any
    # the checkpoint loads as --baseline concept-prune (a full state dict with fp16 entries, strictly)
    E.check_baseline("concept-prune", ckpt_name=ckpt)
    erasure = _script("artist_erasure", "metrics")
    a = erasure.parse_args(["--target", "Monet", "--baseline", "concept-prune", "--base_config_path", tree["yaml"],
                            "--model_id", tree["snap"], "--original_ckpt", tree["ck"] + "/", "--ckpt_name", ckpt, "--tiny"])
    from pdm.utils.load_models import inference_config
    config = inference_config(tree["yaml"], tree["snap"], tiny=True)
    original, erased = E.load_pipelines(config, a, dev)
    got = erased.unet.state_dict()
    for n, v in sd.items():
        assert torch.equal(got[n], v.to(torch.float32)), n
    assert all(torch.equal(v, tree["sd"][n]) for n, v in original.unet.state_dict().items())
