"""ConceptPrune's neuron removal on the GPU (-m gpu): pdmk_wanda_select against the CPU oracle of pdmk_wanda_count taken one
timestep at a time, pdmk_masked_weights against torch.where, `neuron_masks=` in the eager and the captured sampler against a
loop that rewrites the weights with torch, and wanda.py + remove_neurons.py on a tiny snapshot directory.

Every comparison is exact: the feature selects, it computes nothing."""
import hashlib
import importlib.util
import json
import os

import pytest
import torch

import concept_prune_fixtures as fx
import data_fixtures
import neuron_removal_fixtures as nf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16]
CANARY = -1                                                   # 0xFFFFFFFF


def _ids(v):
    return "x".join(str(a) for a in v) if isinstance(v, tuple) else str(v).replace("torch.", "")


# ---------------------------------------------------------------------------------------------- pdmk_wanda_select
def _select(k, w, nb, nt, kk, dev, dtype, pad=0, slack=0, fill=0):
    """int32 [T, O * row_words + slack] (CPU) after one launch on a buffer prefilled with `fill`; pad: columns of 1e4 behind
    every weight row."""
    O, Fd = w.shape
    buf = torch.full((O, Fd + pad), 1e4, device=dev, dtype=dtype)
    buf[:, :Fd] = w.to(dev, dtype)
    bits = torch.full((nt.shape[0], O * k.mask_row_words(Fd) + slack), fill, device=dev, dtype=torch.int32)
    k.wanda_select(buf[:, :Fd], nb.to(dev), nt.to(dev), kk, bits)
    return bits.cpu()


def _unpacked(bits, O, Fd):
    from pdm.utils.concept_prune import unpack_bits
    rw = (Fd + 31) // 32
    return unpack_bits(bits[:, :O * rw].reshape(bits.shape[0], O, rw), Fd)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", fx.COUNT_CASES, ids=_ids)
def test_wanda_select(dev, case, dtype):
    from pdm import _pdmk as k
    from pdm.utils.concept_prune import pack_bits, top_k
    O, Fd, T, ratio = case
    w, nb, nt = fx.count_inputs(O, Fd, T)
    w = w.to(dtype).to(torch.float32)
    kk = top_k(ratio, Fd)
    ref = nf.selection_oracle(w, nb, nt, kk)                          # bool [T, O, F], every t on its own
    slack = 5
    bits = _select(k, w, nb, nt, kk, dev, dtype, slack=slack, fill=CANARY)
    got = _unpacked(bits, O, Fd)
    assert torch.equal(got, ref), int((got != ref).sum())
    words = O * k.mask_row_words(Fd)
    assert torch.equal(bits[:, :words].reshape(T, O, -1), pack_bits(ref))       # overwritten; the bits past F are 0
    assert bool((bits[:, words:] == CANARY).all())                    # t_stride larger than needed: the slack is not touched
    # the sum over t is what pdmk_wanda_count returns on the same inputs
    buf = w.to(dev, dtype)
    count = torch.zeros((O, Fd), device=dev, dtype=torch.int32)
    k.wanda_count(buf, nb.to(dev), nt.to(dev), kk, count)
    assert torch.equal(got.sum(0).to(torch.int32), count.cpu())
    if kk == 0:
        assert int(got.sum()) == 0
    # the same bits from a second launch, whatever the buffer held
    assert torch.equal(_select(k, w, nb, nt, kk, dev, dtype, slack=slack, fill=0)[:, :words], bits[:, :words])


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_wanda_select_ties_zero_rows_and_equal_norms(dev, dtype):
    from pdm import _pdmk as k
    O, Fd, T, kk = 40, 200, 2, 20
    w, nb, nt = fx.tie_inputs(O, Fd, T, kk, dtype)
    assert fx.straddling_ties(w, nt, kk) >= O                         # the tie group lies across the k-th place
    ref = nf.selection_oracle(w, nb, nt, kk)
    got = _unpacked(_select(k, w, nb, nt, kk, dev, dtype, fill=CANARY), O, Fd)
    assert torch.equal(got, ref), int((got != ref).sum())
    assert int(got[:, 1].sum()) <= 3 * T and int(got[:, 1].any(0).sum()) <= 3          # the row with three non-zero weights
    same = torch.arange(8) * (Fd // 8) + 11
    assert int(got[:, :, same].sum()) == 0                            # n_target == n_base: strictly greater, not selected


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_wanda_select_row_stride_and_k_zero(dev, dtype):
    from pdm import _pdmk as k
    w, nb, nt = fx.count_inputs(40, 200, 3)
    w = w.to(dtype).to(torch.float32)
    got = _unpacked(_select(k, w, nb, nt, 20, dev, dtype, pad=24, fill=CANARY), 40, 200)
    assert torch.equal(got, nf.selection_oracle(w, nb, nt, 20))
    zero = _select(k, w, nb, nt, 0, dev, dtype, slack=3, fill=CANARY)         # k = 0 writes zeros (wanda_count returns at once)
    assert int(zero[:, :40 * 7].abs().sum()) == 0 and bool((zero[:, 40 * 7:] == CANARY).all())


def test_wanda_select_rejects(dev):
    from pdm import _pdmk as k
    w = torch.zeros(2, 8200, device=dev)
    n = torch.ones(1, 8200, device=dev)
    bits = torch.zeros(1, 2 * 257, device=dev, dtype=torch.int32)
    with pytest.raises(k.PdmkError):
        k.wanda_select(w, n, n, 10, bits)                              # wider than the kernel keeps on chip
    rc = k._lib.pdmk_wanda_select(w.data_ptr(), k.F32, 2, 8200, 8200, n.data_ptr(), n.data_ptr(), 1, 10, bits.data_ptr(),
                                  2 * 257, None)
    assert rc == -2                                                    # the library's own status
    w, n = torch.zeros(4, 72, device=dev), torch.ones(2, 72, device=dev)
    with pytest.raises(k.PdmkError):
        k.wanda_select(w, n, n, 3, torch.zeros(2, 4 * 3 - 1, device=dev, dtype=torch.int32))       # a word short
    with pytest.raises(k.PdmkError):
        k.wanda_select(w, n, n, 3, torch.zeros(3, 4 * 3, device=dev, dtype=torch.int32))           # T of the norms
    rc = k._lib.pdmk_wanda_select(w.data_ptr(), k.F32, 4, 72, 72, n.data_ptr(), n.data_ptr(), 2, 3, bits.data_ptr(), 11, None)
    assert rc == -1                                                    # t_stride below O * row_words


# ---------------------------------------------------------------------------------------------- pdmk_masked_weights
def _mask_case(k, dev, dtype, layers=nf.MASK_LAYERS, **kw):
    """The arena, its table, the compact pristine copy and random bits (the bits past F set at random as well)."""
    from pdm.utils.concept_prune import pack_bits
    arena, placed = nf.mask_arena(layers, dtype, **kw)
    table = k.MaskTable(placed, dev)
    src = torch.zeros(table.src_elems, dtype=dtype)
    for (d, s, _b, O, _F, ld) in table.layers:
        src[s:s + O * ld] = arena[d:d + O * ld]
    masks = nf.random_masks(layers, nf.MASK_T)
    bits = torch.zeros((nf.MASK_T, table.words + 4), dtype=torch.int32)
    g = torch.Generator().manual_seed(9)
    for (_d, _s, b, O, Fd, _ld), m in zip(table.layers, masks):
        words = pack_bits(m)                                           # [T, O, rw]
        if Fd % 32:
            junk = torch.randint(-2 ** 31, 2 ** 31 - 1, words[..., -1].shape, generator=g, dtype=torch.int64)
            words[..., -1] |= (junk & -(1 << (Fd % 32))).to(torch.int32)
        bits[:, b:b + O * words.shape[-1]] = words.reshape(nf.MASK_T, -1)
    return arena, placed, table, src.to(dev), masks, bits.to(dev)


def _scrambled(arena, placed, dev):
    """The arena on the device with other values in the layers' F columns: what dst holds is not what is written."""
    out = arena.clone()
    for o, O, Fd, ld in placed:
        out[o:o + O * ld].view(O, ld)[:, :Fd] = 7
    return out.to(dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_masked_weights(dev, dtype):
    from pdm import _pdmk as k
    arena, placed, table, src, masks, bits = _mask_case(k, dev, dtype)
    assert table.nrows > len(placed)                                   # a layer in several workgroups

    def run(**kw):
        dst = _scrambled(arena, placed, dev)
        k.masked_weights(dst, src, table, **kw)
        return dst.cpu()

    state = torch.zeros(2, device=dev, dtype=torch.int32)
    want = [nf.masked_arena(arena, placed, masks, t) for t in range(nf.MASK_T)]
    assert not any(torch.equal(want[a], want[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    for t in range(nf.MASK_T):
        got = run(bits=bits, slot=t)
        assert torch.equal(got, want[t]), (t, int((got != want[t]).sum()))        # F columns masked; padding and gaps unchanged
        state[0] = t
        assert torch.equal(run(bits=bits, state=state), want[t])       # the device counter gives the same
        assert torch.equal(run(bits=bits, state=state, slot=1), want[t])          # and wins over the host value
    # repeat_first: calls 0 and 1 are slot 0, call c is slot c - 1
    for call, t in ((0, 0), (1, 0), (2, 1), (3, 2)):
        state[0] = call
        assert torch.equal(run(bits=bits, state=state, repeat_first=True), want[t]), call
    # outside [0, T), or without bits: the pristine weights, bit for bit
    for call, rf in ((3, False), (4, True), (100, False)):
        state[0] = call
        assert torch.equal(run(bits=bits, state=state, repeat_first=rf), arena), call
    for kw in (dict(bits=bits, slot=-1), dict(bits=bits, slot=3), dict(bits=None, slot=0), dict()):
        assert torch.equal(run(**kw), arena), kw


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_masked_weights_unaligned_layers(dev, dtype):
    """An odd width, stride or offset takes the element-wise path (layers at 5 and 480), next to a layer on the 16-byte path
    (at 40)."""
    from pdm import _pdmk as k
    arena, placed, table, src, masks, bits = _mask_case(k, dev, dtype, layers=[(3, 7, 9), (6, 72, 72), (4, 40, 43)], first=5,
                                                        gap=8)
    assert [p[0] for p in placed] == [5, 40, 480]
    for t in range(nf.MASK_T):
        dst = _scrambled(arena, placed, dev)
        k.masked_weights(dst, src, table, bits=bits, slot=t)
        assert torch.equal(dst.cpu(), nf.masked_arena(arena, placed, masks, t)), t
    dst = _scrambled(arena, placed, dev)
    k.masked_weights(dst, src, table)
    assert torch.equal(dst.cpu(), arena)


def test_masked_weights_in_a_master_arena(dev):
    """fp32: the arena the engine reads is the master itself.  Masks are always made from the pristine copy - a weight masked at
    one slot is back at the next - and the restore leaves the arena as it was."""
    from pdm import _pdmk as k
    arena, placed, table, _src, masks, bits = _mask_case(k, dev, torch.float32)
    master = arena.to(dev)
    pristine = torch.zeros(table.src_elems, device=dev)
    for (d, s, _b, O, _F, ld) in table.layers:                        # attach
        pristine[s:s + O * ld].copy_(master[d:d + O * ld])
    for t in (1, 2, 0):                                               # apply, in place
        k.masked_weights(master, pristine, table, bits=bits, slot=t)
        assert torch.equal(master.cpu(), nf.masked_arena(arena, placed, masks, t)), t
    k.masked_weights(master, pristine, table)                         # detach
    assert torch.equal(master.cpu(), arena)


def test_masked_weights_rejects(dev):
    from pdm import _pdmk as k
    arena, placed, table, src, masks, bits = _mask_case(k, dev, torch.float32)
    dst = arena.to(dev)
    with pytest.raises(k.PdmkError):
        k.masked_weights(dst[:table.extent - 1], src, table, bits=bits, slot=0)
    with pytest.raises(k.PdmkError):
        k.masked_weights(dst, src[:-8], table, bits=bits, slot=0)
    with pytest.raises(k.PdmkError):
        k.masked_weights(dst, src.to(torch.bfloat16), table, bits=bits, slot=0)
    with pytest.raises(k.PdmkError):
        k.masked_weights(dst, src, table, bits=bits[:, :table.words - 1], slot=0)
    with pytest.raises(k.PdmkError):
        k.masked_weights(dst, src, table, bits=bits, state=torch.zeros(1, device=dev, dtype=torch.int64))
    assert torch.equal(dst.cpu(), arena)


# ---------------------------------------------------------------------------------------------- the sampler
STEPS, RATIO = 3, 0.25


def _scheduler(name):
    from pdm.pipelines.pruning_pipelines import DDIMScheduler, PNDMScheduler
    return DDIMScheduler(prediction_type="v_prediction") if name == "ddim" else PNDMScheduler(prediction_type="epsilon")


def _oracle_masks(unet, layers, base, target):
    """[bool [T, O, F]] from the CPU oracle on the fp32 master weights: no kernel of the feature has a hand in it."""
    from pdm.utils.concept_prune import top_k
    out = []
    for (key, O, Fd, _fp), nb, nt in zip(layers, base, target):
        e = unet.store.by_key[key + ".weight"]
        w = unet.store.p(key + ".weight").view(e.shape)[:O, :Fd].cpu()
        out.append(nf.selection_oracle(w, nb, nt, top_k(RATIO, Fd)))
    return out


class _TorchRemover:
    """The independent loop: the sampler's eager loop with a callback that rewrites the layers' compute weights with torch
    before the next U-Net call (callback i follows scheduler step i, so it prepares call i + 1)."""

    def __init__(self, unet, layers, masks, repeat_first, ncalls):
        self.unet, self.layers, self.masks, self.repeat_first, self.ncalls = unet, layers, masks, repeat_first, ncalls
        self.saved = unet.store.w.clone()
        self.set(0)

    def set(self, call):
        slot = max(call - 1, 0) if self.repeat_first else call
        st = self.unet.store
        for (key, O, Fd, _fp), m in zip(self.layers, self.masks):
            e = st.by_key[key + ".weight"]
            pristine = self.saved[e.off:e.off + e.numel].view(e.shape)[:O, :Fd]
            st.w[e.off:e.off + e.numel].view(e.shape)[:O, :Fd] = torch.where(m[slot].to(pristine.device), 0, pristine)

    def __call__(self, i, t, latents):
        if i + 1 < self.ncalls:
            self.set(i + 1)

    def restore(self):
        self.unet.store.w.copy_(self.saved)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("sched", ["ddim", "pndm"])
def test_neuron_masks_in_the_sampler(dev, dtype, sched, monkeypatch):
    from pdm.utils import concept_prune as CP
    pipe = nf.pipe(dev, dtype, _scheduler(sched))
    unet, st = pipe.unet, pipe.unet.store
    pe, ne, lat = nf.sampling_inputs()
    layers = CP.ffn_layers(unet)
    base, target = nf.norm_sets(layers, STEPS)
    w0, m0 = st.w.clone(), st.master.clone()

    def run(steps=STEPS, **kw):
        out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=steps, guidance_scale=7.5,
                   output_type="latent", **kw).images
        assert torch.equal(st.w, w0) and torch.equal(st.master, m0)    # after every call the arenas are what they were
        return out

    masks = CP.TimestepMasks.from_norms(unet, base, target, RATIO)
    oracle = _oracle_masks(unet, layers, base, target)
    for l, (key, O, Fd, _fp) in enumerate(layers):                    # the masks the sampler gets are the oracle's
        assert torch.equal(CP.unpack_bits(masks.layer_bits(l), Fd).cpu(), oracle[l]), key
        assert masks.density()[key] == [int(oracle[l][t].sum()) / (O * Fd) for t in range(STEPS)]
    assert sum(int(m.sum()) for m in oracle) > 0 and not torch.equal(oracle[0][0], oracle[0][STEPS - 1])

    plain = run()
    captured = run(neuron_masks=masks)
    assert pipe.captures == (1 if sched == "ddim" else 2)             # DDIM: the plain loop is eager, the masked one captured
    assert pipe._use_graph(True if sched == "ddim" else None, None)
    n = pipe.captures
    again = run(neuron_masks=masks)
    assert pipe.captures == n and torch.equal(again, captured)        # a second call replays the same capture
    monkeypatch.setenv("PDMK_SAMPLER_GRAPH", "0")
    eager = run(neuron_masks=masks)
    assert pipe.captures == n
    monkeypatch.delenv("PDMK_SAMPLER_GRAPH")
    assert torch.equal(captured, eager)                                # bit-identical loops
    assert not torch.equal(captured, plain)                            # and the masks do something

    ncalls = STEPS + (1 if sched == "pndm" else 0)
    remover = _TorchRemover(unet, layers, oracle, sched == "pndm", ncalls)
    try:
        ref = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=STEPS, guidance_scale=7.5,
                   output_type="latent", callback=remover).images
    finally:
        remover.restore()
    assert torch.equal(st.w, w0) and torch.equal(st.master, m0)
    assert torch.equal(captured, ref) and torch.equal(eager, ref)

    zeros = CP.TimestepMasks(unet, STEPS)                              # all-zero masks: sampling without the keyword
    assert torch.equal(run(neuron_masks=zeros), plain)
    assert pipe.captures == n + 1                                      # other masks, another capture
    monkeypatch.setenv("PDMK_SAMPLER_GRAPH", "0")
    assert torch.equal(run(neuron_masks=zeros), plain)
    monkeypatch.delenv("PDMK_SAMPLER_GRAPH")

    with pytest.raises(ValueError, match="timesteps"):                 # T of the masks against the steps of the call
        run(steps=STEPS + 1, neuron_masks=masks)
    assert torch.equal(st.w, w0) and torch.equal(st.master, m0) and not masks.attached


def test_neuron_masks_restore_on_error_and_context_manager(dev):
    from pdm.utils import concept_prune as CP
    pipe = nf.pipe(dev, torch.float32, _scheduler("ddim"))
    unet, st = pipe.unet, pipe.unet.store
    pe, ne, lat = nf.sampling_inputs()
    layers = CP.ffn_layers(unet)
    masks = CP.TimestepMasks.from_norms(unet, *nf.norm_sets(layers, STEPS), RATIO)
    w0 = st.w.clone()
    with pytest.raises(RuntimeError, match="attach"):
        masks.apply(slot=0)
    with pytest.raises(ZeroDivisionError):
        with masks.attach():
            masks.apply(slot=1)
            assert not torch.equal(st.w, w0) and st.w is st.master    # fp32: the master arena itself is masked
            1 / 0
    assert torch.equal(st.w, w0) and not masks.attached

    def boom(i, t, latents):                                          # an error in the middle of the eager loop
        assert not torch.equal(st.w, w0)
        raise KeyError("boom")
    with pytest.raises(KeyError):
        pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=STEPS, guidance_scale=7.5,
             output_type="latent", callback=boom, neuron_masks=masks)
    assert torch.equal(st.w, w0) and not masks.attached


def test_neuron_masks_raise_with_lms_sld_and_algebra(dev):
    from pdm.pipelines.pruning_pipelines import LMSDiscreteScheduler
    from pdm.utils import concept_prune as CP
    pipe = nf.pipe(dev, torch.float32, _scheduler("ddim"))
    pe, ne, lat = nf.sampling_inputs()
    masks = CP.TimestepMasks(pipe.unet, STEPS)
    w0 = pipe.unet.store.w.clone()
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=STEPS, guidance_scale=7.5,
              output_type="latent", neuron_masks=masks)
    g = torch.Generator().manual_seed(8)
    with pytest.raises(ValueError, match="SLD"):
        pipe(safety_concept_embeds=torch.randn(1, 13, 64, generator=g), **kw)
    with pytest.raises(ValueError, match="concept algebra"):
        pipe(algebra_embeds=torch.randn(3, 13, 64, generator=g), **kw)
    other = nf.pipe(dev, torch.float32, _scheduler("ddim"))
    with pytest.raises(ValueError, match="another U-Net"):
        other(**kw)
    pipe.scheduler = LMSDiscreteScheduler(prediction_type="epsilon")
    with pytest.raises(NotImplementedError, match="LMS"):
        pipe(**kw)
    assert pipe.captures == 0 and torch.equal(pipe.unet.store.w, w0) and not masks.attached


# ---------------------------------------------------------------------------------------------- the scripts, tiny snapshot
def _script(name):
    spec = importlib.util.spec_from_file_location(name + "_nr_gpu", os.path.join(ROOT, "unlearn-ft_amd", "scripts", "baselines",
                                                                                "concept_prune", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _digest(folder):
    h = hashlib.sha256()
    for base, _dirs, files in sorted(os.walk(folder)):
        for n in sorted(files):
            h.update(os.path.relpath(os.path.join(base, n), folder).encode())
            with open(os.path.join(base, n), "rb") as f:
                h.update(f.read())
    return h.hexdigest()


def test_scripts_on_a_tiny_snapshot(dev, tmp_path):
    from PIL import Image
    from pdm.utils import concept_prune as CP
    tree = data_fixtures.write_pruned_checkpoint_tree(str(tmp_path), dev, "cp.yaml")
    words = os.path.join(tree["root"], "words")
    os.makedirs(words)
    with open(os.path.join(words, "things.txt"), "w") as f:
        f.write("cat\ndog\n")
    T, ratio = 3, 0.25
    argv = ["--target", "Monet", "--base_config_path", tree["yaml"], "--model_id", tree["snap"], "--ckpt_path", tree["ck"] + "/",
            "--result_dir", os.path.join(tree["root"], "res"), "--words_dir", words, "--timesteps", str(T),
            "--skill_ratio", str(ratio), "--image_resolution", "64", "--tiny", "--seed", "0"]
    before = _digest(tree["ck"])
    _script("wanda").main(argv)
    out = _script("remove_neurons").main(argv)
    res = os.path.join(tree["root"], "res", "snapshot", "Monet")
    assert out == os.path.join(res, "after_removal_results", str(ratio))
    names = [f"img_{i}_a {w} in the style of Monet.jpg" for i, w in enumerate(("cat", "dog"))]
    assert sorted(os.listdir(out)) == sorted(names + ["mask_density.json"])
    for n in names:
        with Image.open(os.path.join(out, n)) as im:
            assert im.size == (530, 290)
    base, target = (CP.load_norms(os.path.join(res, n)) for n in ("base_norms.pt", "target_norms.pt"))
    want = {}
    for l, n in enumerate(n for n in tree["sd"] if n.endswith("ff.net.2.weight")):
        w = tree["sd"][n]
        sel = nf.selection_oracle(w, base[l], target[l], CP.top_k(ratio, w.shape[1]))
        want[n[:-len(".weight")]] = [int(sel[t].sum()) / w.numel() for t in range(T)]
    with open(os.path.join(out, "mask_density.json")) as f:
        got = json.load(f)
    assert list(got) == list(want) and got == want
    assert any(d > 0 for v in want.values() for d in v)
    assert _digest(tree["ck"]) == before                              # the checkpoint is read, never written
