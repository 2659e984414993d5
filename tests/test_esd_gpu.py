"""ESD on the engine (-m gpu): the captured DDIM loop with an early stop against the eager one, one training step and three whole
iterations against the CPU oracle (tests/esd_fixtures.py), and the script.  Tiny topology, 16 x 16 latents, 13 text tokens.

Bounds of the step and the loop are the ones the same engine is held to in tests/test_step_parity_gpu.py
(test_upper_step_matches_oracle: fp32 loss 2e-4 relative, gradients 2e-3 of the tensor's scale; bf16 loss 3e-2, cosine > 0.98 on
tensors of >= 4096 elements; test_bilevel_loss_curve_matches_oracle: 1e-3 / 2e-2 per loss): the arithmetic is the upper step's
with one more frozen row.
"""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unlearn-ft_amd", "scripts", "baselines",
                      "erasing", "esd_diffusers.py")
_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def tree(dev, tmp_path_factory):
    import data_fixtures as F
    return F.write_pruned_checkpoint_tree(str(tmp_path_factory.mktemp("esd")), dev, "esd.yaml")


@pytest.fixture(scope="module")
def oracle(tree):
    import esd_fixtures as X
    return X.oracle_model(tree)


def _models(tree, dev, dn):
    from pdm.utils.load_models import FrozenModels, inference_config
    models = FrozenModels(inference_config(tree["yaml"], tiny=True, mixed_precision="no" if dn == "f32" else "bf16"), dev)
    assert models.weight_dtype == _DT[dn]
    return models


def _trainer(tree, dev, dn, method, **kw):
    from pdm.training.esd import EsdTrainer
    models = _models(tree, dev, dn)
    frozen, student = models.load_unet(tree["ck"]), models.load_unet(tree["ck"], train=True)
    assert not frozen.store.train and student.store.train
    pipe = models.pipeline(student, kind="ddim", tokenizer=False)
    return EsdTrainer(frozen, student, pipe, method, **kw)


def _rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)


# ------------------------------------------------------------------------------------------------ captured = eager
@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_captured_ddim_loop_equals_eager_and_follows_the_weights(dev, tree, dn):
    from pdm.pipelines.pruning_pipelines import DDIMScheduler
    models = _models(tree, dev, dn)
    student = models.load_unet(tree["ck"], train=True)
    pipe = models.pipeline(student, kind="ddim", tokenizer=False)
    assert type(pipe.scheduler) is DDIMScheduler
    g = torch.Generator().manual_seed(11)
    pe, ne = torch.randn(1, 13, 64, generator=g), torch.randn(1, 13, 64, generator=g)
    lat = torch.randn(1, 4, 16, 16, generator=g)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=5, guidance_scale=3.0,
              output_type="latent")
    full = pipe(graph=None, **kw).images                       # graph=None: a DDIM scheduler stays on the eager loop
    assert pipe.captures == 0 and not pipe._loops
    assert torch.equal(full, pipe(graph=False, **kw).images)
    ends = {}
    for n, end in enumerate((1, 3, 5)):
        e = pipe(graph=False, end_iteration=end, **kw).images
        c = pipe(graph=True, end_iteration=end, **kw).images
        assert torch.equal(e, c), end
        assert pipe.captures == 1, "the second and third calls replay the first capture"
        ends[end] = e
    assert torch.equal(ends[5], full) and not torch.equal(ends[1], ends[3]) and not torch.equal(ends[3], ends[5])
    assert torch.equal(pipe(graph=True, **kw).images, full)
    # the optimiser rewrites the weights in place: the same capture follows them
    store = student.store
    pg = torch.Generator(device=dev).manual_seed(5)
    store.master.mul_(1.0 + 0.05 * torch.randn(store.total, device=dev, generator=pg))
    store.refresh()
    e = pipe(graph=False, end_iteration=3, **kw).images
    c = pipe(graph=True, end_iteration=3, **kw).images
    assert pipe.captures == 1 and torch.equal(e, c) and not torch.equal(e, ends[3])
    with pytest.raises(ValueError):
        pipe(graph=True, end_iteration=6, **kw)


# ------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("method", ["xattn", "noxattn"])
@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_one_step_matches_oracle(dev, tree, oracle, dn, method, same):
    import esd_fixtures as X
    ocfg, info, sd0 = oracle
    lr, ng, t = 1e-3, 1.0, 400
    x, emb_p, emb_n, emb_f = X.inputs()
    P = {n: v.clone().requires_grad_(True) for n, v in sd0.items()}
    loss, (e_p, e_n, _) = X.esd_loss(P, sd0, ocfg, info, x, t, emb_p, emb_n, emb_f, same, ng)
    assert float((e_p - e_n).abs().max()) >= 0.05 * float(e_p.abs().max())
    loss.backward()
    tr = _trainer(tree, dev, dn, method, lr=lr, negative_guidance=ng)
    names = set(tr.names)
    assert names and names < set(sd0) and all(("attn2" in n) == (method == "xattn") for n in names)
    assert not [n for n in names if "norm" in n]
    got = float(tr.loss_and_grads(x.to(dev), t, emb_p, emb_n, emb_f, same).item())
    ltol = 2e-4 if dn == "f32" else 3e-2
    print(f"esd step {dn} {method} same={same}: loss {got:.6e} oracle {loss.item():.6e} rel "
          f"{abs(got - loss.item()) / abs(loss.item()):.2e}")
    assert abs(got - loss.item()) <= ltol * abs(loss.item()), (got, loss.item())
    store = tr.student.store
    grads = store.state_dict(arena=store.grad)
    if dn == "f32":
        worst = max((_rel(grads[n], P[n].grad), n) for n in names)
        print(f"   worst trainable gradient distance {worst[0]:.2e} ({worst[1]})")
        assert worst[0] < 2e-3, worst
    else:
        big = [n for n in names if P[n].numel() >= 4096]
        cos = min(torch.nn.functional.cosine_similarity(grads[n].flatten(), P[n].grad.flatten(), dim=0).item() for n in big)
        print(f"   smallest cosine over {len(big)} trainable tensors {cos:.4f}")
        assert big and cos > 0.98, cos
    # the optimiser: torch.optim.Adam on the subset
    before = tr.student.state_dict()
    assert all(torch.equal(before[n], sd0[n]) for n in sd0)
    opt = torch.optim.Adam([P[n] for n in sorted(names)], lr=lr)
    opt.step()
    tr.opt.step(grad_scale=1.0, zero_grad=True)
    after = tr.student.state_dict()
    frozen_names = set(sd0) - names
    assert all(torch.equal(after[n], sd0[n]) for n in frozen_names), "a tensor outside the subset moved"
    assert all(not torch.equal(after[n], sd0[n]) for n in names), "a trainable tensor did not move"
    if dn == "f32":
        worst = 0.0
        for n in names:
            gr = P[n].grad
            mask = gr.abs() > 1e-3 * gr.abs().max()
            d_ref, d_got = (P[n].detach() - sd0[n])[mask], (after[n] - sd0[n])[mask]
            worst = max(worst, (d_got - d_ref).abs().max().item() / lr)
        print(f"   worst first-step delta distance {worst:.2e} lr")
        assert worst < 2e-2, worst
    for off, n in tr.segments:
        assert float(store.grad[off:off + n].abs().max()) == 0.0
    assert float(store.grad.abs().max()) > 0.0                 # the frozen entries' gradients are left as they are
    if dn == "bf16":                                           # the compute copy follows the master inside the subset
        assert torch.equal(store.w, store.master.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ the loop
@pytest.mark.parametrize("dn,tol", [("f32", 1e-3), ("bf16", 2e-2)])
def test_three_iterations_match_oracle(dev, tree, oracle, dn, tol):
    import esd_fixtures as X
    from pdm.pipelines.pruning_pipelines import DDIMScheduler
    from pdm.utils import esd as E
    ocfg, info, sd0 = oracle
    lr, ng, nsteps = 1e-3, 1.0, 5
    pairs = [["a", "a"], ["b", "c"]]
    g = torch.Generator().manual_seed(3)
    embs = {text: torch.randn(1, 13, 64, generator=g) for text in ("", "a", "b", "c")}
    np.random.seed(0)
    torch.manual_seed(0)
    gen = E.draws(len(pairs), nsteps, (1, 4, 16, 16))
    draws = [next(gen) for _ in range(3)]
    assert all(1 <= it <= 3 for _, it, _ in draws)
    tr = _trainer(tree, dev, dn, "xattn", lr=lr, negative_guidance=ng, nsteps=nsteps, graph=True)
    tr._emb.update({text: e.to(dev) for text, e in embs.items()})
    got = [float(tr.iteration(pairs, d).item()) for d in draws]
    assert tr.pipe.captures == 1
    # the same loop on the oracle
    P = {n: v.clone().requires_grad_(True) for n, v in sd0.items()}
    opt = torch.optim.Adam([P[n] for n in tr.names], lr=lr)
    sch = DDIMScheduler(prediction_type="v_prediction")
    want = []
    for index, it, latents in draws:
        concept, erase_from = pairs[index]
        x = X.partial_sampling(P, ocfg, info, sch, latents, embs[concept], embs[""], nsteps, it)
        t = 1000 - 200 * it
        assert t == tr.t_of[it]
        opt.zero_grad()
        loss, _ = X.esd_loss(P, sd0, ocfg, info, x, t, embs[concept], embs[""], embs[erase_from], concept == erase_from, ng)
        loss.backward()
        opt.step()
        want.append(loss.item())
    rel = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    print(f"esd loop {dn}: losses {got} oracle {want} rel {rel}")
    assert max(rel) <= tol, (got, want)


# ------------------------------------------------------------------------------------------------ the script
def _script():
    spec = importlib.util.spec_from_file_location("esd_diffusers_script", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_writes_the_reference_checkpoint(dev, tree, tmp_path):
    from pdm.training.esd import train
    from pdm.utils import erasure_utils as R
    from pdm.utils import esd as E
    mod = _script()

    def argv(out, graph):
        return ["--erase_concept", "the thing, and", "--erase_from", "of", "--train_method", "xattn", "--iterations", "3",
                "--tiny", "--image_size", "128", "--lr", "1e-3", "--base_config_path", tree["yaml"], "--ckpt_path", tree["ck"],
                "--save_path", str(tmp_path / out), "--graph", str(graph), "--seed", "0", "--log_every", "0"]
    args = mod.parse_args(argv("a", 0))
    path, tr = train(args, log=lambda *a: None)
    assert path == str(tmp_path / "a") + "/esd-thethingand_from_of-xattn_1-epochs_3.pt" and os.path.exists(path)
    nested = torch.load(path, map_location="cpu")
    names, kinds = E.entry_names(tr.student.store.entries)
    want = E.trainable_names(names, kinds, "xattn")
    assert set(nested) == {"unet." + n.rsplit(".", 1)[0] for n in want}
    assert sum(len(v) for v in nested.values()) == len(want)
    assert all(t.dtype == torch.float32 and t.device.type == "cpu" for v in nested.values() for t in v.values())
    trained = tr.student.state_dict()
    assert any(not torch.equal(trained[n], tree["sd"][n]) for n in want)
    # the evaluation side reads it back into the trained student
    models = _models(tree, dev, "f32")
    loaded = R.load_erasure_checkpoint(models.load_unet(tree["ck"]), path, esd=True).state_dict()
    assert set(loaded) == set(trained) and all(torch.equal(loaded[n], trained[n]) for n in trained)
    ns = SimpleNamespace(original_ckpt=tree["ck"], baseline="esd", ckpt_name=path)
    original, erased = R.load_pipelines(models.config, ns, dev)
    got = erased.unet.state_dict()
    assert all(torch.equal(got[n], trained[n]) for n in trained)
    assert all(torch.equal(original.unet.state_dict()[n], tree["sd"][n]) for n in trained)
    # the same seed twice gives the same bytes; the captured loop gives the eager loop's
    data = open(path, "rb").read()
    for out, graph in (("b", 0), ("c", 1)):
        again = mod.main(argv(out, graph))
        assert os.path.basename(again) == os.path.basename(path)
        assert open(again, "rb").read() == data, (out, graph)


def test_script_refuses_the_two_methods_before_loading(tmp_path):
    mod = _script()
    base = ["--erase_concept", "x", "--save_path", str(tmp_path), "--ckpt_path", str(tmp_path / "nothing")]
    with pytest.raises(ValueError, match="empty parameter list"):
        mod.main(base + ["--train_method", "xattn-strict"])
    with pytest.raises(NotImplementedError):
        mod.main(base + ["--train_method", "full"])
