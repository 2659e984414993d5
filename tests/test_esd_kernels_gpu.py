"""The three kernels ESD adds (-m gpu): pdmk_ddim_step bit-identical to the eager chain it replaces, pdmk_adamw_segments
bit-identical to pdmk_adamw on the gathered elements and silent outside them, pdmk_esd_head against fp64.

pdmk_esd_head's bounds are the project's rule: the kernel may be 4 x d_ref from fp64, d_ref being the distance from fp64 of the
fp32 torch chain `mse_loss(pred, e_f - ng * (e_p - e_n))` with its autograd gradient on the same inputs - for the loss the
relative distance, for the seed max |difference| over max |fp64 seed|.  With bf16 storage the seed is a bf16 number: it may
differ from the bf16-rounded fp64 seed by one bf16 ulp.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ pdmk_ddim_step
def _eager_chain(sch, i, pred, ld, B, C, H, W, cfg, g, lat, dtype, cp):
    """What generate_samples' eager loop does between two U-Net calls with a DDIMScheduler: NHWC -> NCHW, guidance axpby,
    DDIMScheduler.step, the doubled latent copy and nchw_to_nhwc.  Returns (new latents, next U-Net input)."""
    from pdm import _pdmk as k
    R = 2 * B if cfg else B
    out = torch.empty(R, C, H, W, device=lat.device)
    k.nhwc_to_nchw(pred, out, R, C, H * W, ld)
    if cfg:
        noise = out[B:]
        k.axpby(out[:B], noise, 1.0 - g, g)
    else:
        noise = out
    lat = sch.step(noise.contiguous(), int(sch.timesteps[i]), lat, return_dict=False)[0]
    x2 = torch.cat([lat, lat]) if cfg else lat
    x = torch.empty(R * H * W, cp, device=lat.device, dtype=dtype)
    k.nchw_to_nhwc(x2.contiguous(), x, R, C, H * W, cp)
    return lat, x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_ddim_step_equals_eager_chain(dev, dtype, cfg, prediction_type):
    from pdm import _pdmk as k
    from pdm.pipelines.pruning_pipelines import DDIMScheduler
    from pdm.models.unet.spec import padc
    B, C, H, W, g = 2, 4, 8, 12, 3.0
    cp, ld = padc(C), padc(C) + 8                     # the prediction's row stride differs from the input's
    R = 2 * B if cfg else B
    for steps in (1, 2, 3, 50):
        gen = torch.Generator(device=dev).manual_seed(steps)
        sch = DDIMScheduler(prediction_type=prediction_type)
        sch.set_timesteps(steps)
        rows = sch.ddim_rows()
        N = len(rows)
        assert N == steps and ctypes.sizeof(k.DdimRow) == 24
        table = k.ddim_table(rows, dev)
        lat0 = torch.randn(B, C, H, W, device=dev, generator=gen)
        sample = lat0.reshape(-1).clone()
        state = torch.zeros(2, device=dev, dtype=torch.int32)
        t_out = torch.zeros(R, device=dev, dtype=torch.int64)
        x_next = torch.full((R * H * W, cp), 3.0, device=dev, dtype=dtype)      # padding must come back as zeros
        lat = lat0.clone()
        for i in range(N):
            pred = (torch.randn(R * H * W, ld, device=dev, generator=gen) * 2).to(dtype)
            lat, x_ref = _eager_chain(sch, i, pred, ld, B, C, H, W, cfg, g, lat, dtype, cp)
            k.ddim_step(pred, ld, 1.0 - g, g, cfg, sample, table, N, state, t_out, x_next, cp, B, C, H * W)
            what = f"steps {steps}, step {i}"
            assert torch.equal(sample.view(B, C, H, W), lat), what
            assert torch.equal(x_next, x_ref), what
            assert state.tolist() == [i + 1, 0], what
            if i + 1 < N:
                assert t_out.tolist() == [int(sch.timesteps[i + 1])] * R, what
        # a launch past the end of the table changes nothing
        before = [t.clone() for t in (sample, x_next, state, t_out)]
        k.ddim_step(pred, ld, 1.0 - g, g, cfg, sample, table, N, state, t_out, x_next, cp, B, C, H * W)
        assert all(torch.equal(a, b) for a, b in zip(before, (sample, x_next, state, t_out)))


# ------------------------------------------------------------------------------------------------ pdmk_adamw_segments
def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _many_segments(total_blocks, seed=0):
    """~300 segments of 128 ... 5120 elements with gaps of 0 ... 3 blocks (a gap of 0 makes two of them adjacent)."""
    g = torch.Generator().manual_seed(seed)
    segs, blk = [], 1
    while len(segs) < 300:
        n = int(torch.randint(1, 41, (1,), generator=g))
        if blk + n > total_blocks:
            break
        segs.append((blk * 128, n * 128))
        blk += n + int(torch.randint(0, 4, (1,), generator=g))
    return segs


_ARENA = 128 * 37
_TABLES = {
    "first_block": (_ARENA, [(0, 128)], None),
    "to_the_end": (_ARENA, [(128 * 30, 128 * 7)], None),
    "two_adjacent": (_ARENA, [(128 * 3, 128 * 2), (128 * 5, 128 * 4)], None),
    "many": (128 * 7000, _many_segments(7000), None),
    "many_cut": (128 * 7000, _many_segments(7000), 1024),        # segments longer than a table row are cut into several
    "whole": (_ARENA, [(0, _ARENA)], None),
    "whole_cut": (_ARENA, [(0, _ARENA)], 512),
}


@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("case", list(_TABLES))
def test_adamw_segments_equals_adamw_on_the_gathered_copy(dev, case, step, with_w):
    from pdm import _pdmk as k
    total, segs, row = _TABLES[case]
    if case.startswith("many"):
        assert 250 <= len(segs) <= 300 and max(n for _, n in segs) == 5120 and min(n for _, n in segs) == 128
    table = k.AdamwTable(segs, dev) if row is None else k.AdamwTable(segs, dev, row=row)
    if row is not None:
        assert table.nrows > len(segs)
    ncomp = sum(n for _, n in segs)
    assert table.compact == ncomp
    gen = torch.Generator(device=dev).manual_seed(step)
    idx = torch.cat([torch.arange(o, o + n) for o, n in segs]).to(dev)
    inside = torch.zeros(total, dtype=torch.bool, device=dev)
    inside[idx] = True
    nan = float("nan")
    p = torch.full((total,), nan, device=dev)
    g = torch.full((total,), nan, device=dev)
    w = torch.full((total,), nan, device=dev, dtype=torch.bfloat16) if with_w else None
    p[idx] = torch.randn(ncomp, device=dev, generator=gen)
    g[idx] = torch.randn(ncomp, device=dev, generator=gen) * 0.1
    if step == 1:
        m, v = torch.zeros(ncomp, device=dev), torch.zeros(ncomp, device=dev)
    else:
        m = torch.randn(ncomp, device=dev, generator=gen) * 0.05
        v = torch.rand(ncomp, device=dev, generator=gen) * 0.01
    b1, b2, eps, wd = 0.9, 0.999, 1e-8, 0.01
    lr = torch.tensor([1e-3], device=dev)
    bc = torch.tensor([1 - b1 ** step, 1 - b2 ** step], device=dev)
    # the gathered contiguous copy through pdmk_adamw
    pc, gc, mc, vc = p[idx].clone(), g[idx].clone(), m.clone(), v.clone()
    wc = torch.zeros(ncomp, device=dev, dtype=torch.bfloat16) if with_w else None
    k.adamw(pc, gc, mc, vc, ncomp, lr, b1, b2, eps, wd, bc, 0.5, False, w_bf16=wc)
    p0, g0 = p.clone(), g.clone()
    w0 = w.clone() if with_w else None
    k.adamw_segments(p, g, m, v, table, lr, b1, b2, eps, wd, bc, 0.5, False, w_bf16=w)
    assert torch.equal(_bits(p[idx]), _bits(pc)) and torch.equal(_bits(m), _bits(mc)) and torch.equal(_bits(v), _bits(vc))
    assert torch.equal(_bits(g), _bits(g0)), "zero_grad off: the gradients stay"
    assert not torch.isnan(p[idx]).any() and not torch.equal(p[idx], p0[idx])
    assert torch.equal(_bits(p)[~inside], _bits(p0)[~inside])
    if with_w:
        assert torch.equal(_bits(w[idx]), _bits(wc)) and torch.equal(_bits(w)[~inside], _bits(w0)[~inside])
    # a second step, clearing the gradients: inside only
    k.adamw(pc, gc, mc, vc, ncomp, lr, b1, b2, eps, wd, bc, 0.5, True, w_bf16=wc)
    k.adamw_segments(p, g, m, v, table, lr, b1, b2, eps, wd, bc, 0.5, True, w_bf16=w)
    assert torch.equal(_bits(p[idx]), _bits(pc)) and torch.equal(_bits(m), _bits(mc)) and torch.equal(_bits(v), _bits(vc))
    assert float(gc.abs().max()) == 0.0 and float(g[idx].abs().max()) == 0.0
    assert torch.equal(_bits(g)[~inside], _bits(g0)[~inside]) and torch.equal(_bits(p)[~inside], _bits(p0)[~inside])
    if with_w:
        assert torch.equal(_bits(w[idx]), _bits(wc)) and torch.equal(_bits(w)[~inside], _bits(w0)[~inside])


def test_adamw_segments_rejects(dev):
    from pdm import _pdmk as k
    n = 1024
    p, g, m, v = (torch.zeros(n, device=dev) for _ in range(4))
    lr, bc = torch.tensor([1e-3], device=dev), torch.tensor([0.1, 0.001], device=dev)
    table = k.AdamwTable([(0, 128)], dev)
    st = torch.cuda.current_stream().cuda_stream

    def raw(pp, tab, nseg):
        return k._lib.pdmk_adamw_segments(pp, g.data_ptr(), m.data_ptr(), v.data_ptr(), tab, nseg, lr.data_ptr(), 0.9, 0.999,
                                          1e-8, 0.0, bc.data_ptr(), 1.0, 0, None, st)
    assert raw(p.data_ptr(), table.dev.data_ptr(), 0) == -1
    assert raw(p.data_ptr(), table.dev.data_ptr(), -3) == -1
    assert raw(p.data_ptr(), None, 1) == -1
    assert raw(None, table.dev.data_ptr(), 1) == -1
    assert raw(p.data_ptr() + 4, table.dev.data_ptr(), 1) == -1           # arena not 16-byte aligned
    for bad in ([(2, 128)], [(0, 126)], [(0, 0)], [(-4, 8)], [(0, 128), (64, 128)], []):
        with pytest.raises(k.PdmkError):
            k.AdamwTable(bad, dev)
    with pytest.raises(k.PdmkError):                                        # a table that reaches past the arena
        k.adamw_segments(p, g, m, v, k.AdamwTable([(n - 64, 128)], dev), lr, 0.9, 0.999, 1e-8, 0.0, bc, 1.0, False)
    with pytest.raises(k.PdmkError):                                        # moments shorter than the compact length
        k.adamw_segments(p, g, m[:64], v, table, lr, 0.9, 0.999, 1e-8, 0.0, bc, 1.0, False)
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ pdmk_esd_head
def _bf16_steps(a, b):
    """|a - b| in units of bf16 steps (sign-magnitude bit patterns made monotonic)."""
    def mono(t):
        x = t.view(torch.int16).int()
        return torch.where(x < 0, -(x & 0x7FFF), x)
    return (mono(a) - mono(b)).abs().max().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("ng", [1.0, 0.5, 3.0])
@pytest.mark.parametrize("rows", [1, 77, 1024])
def test_esd_head_against_fp64(dev, rows, ng, alias, dtype):
    from pdm import _pdmk as k
    cols, ldp, lde = 4, 8, 16
    gen = torch.Generator().manual_seed(rows)
    pred = torch.randn(rows, ldp, generator=gen).to(dtype)                # bf16 storage: bf16-representable values
    e = torch.randn(3 * rows, lde, generator=gen).to(dtype)
    e_p, e_n = e[:rows], e[rows:2 * rows]
    e_f = e_n if alias else e[2 * rows:]
    n = rows * cols

    def chain(t):
        pr = pred[:, :cols].to(t).clone().requires_grad_(True)
        tgt = e_f[:, :cols].to(t) - ng * (e_p[:, :cols].to(t) - e_n[:, :cols].to(t))
        loss = torch.nn.functional.mse_loss(pr, tgt)
        loss.backward()
        return loss.detach(), pr.grad
    loss64, g64 = chain(torch.float64)
    loss32, g32 = chain(torch.float32)
    d_ref_loss = abs(float(loss32.double() - loss64)) / float(loss64)
    d_ref_seed = float((g32.double() - g64).abs().max()) / float(g64.abs().max())

    predd, ed = pred.to(dev), e.to(dev)
    out = torch.zeros(2, device=dev, dtype=torch.float64)
    dpred = torch.full((rows, ldp), 3.0, device=dev, dtype=dtype)
    k.esd_head(predd, ed[:rows], ed[rows:2 * rows], ed[rows:2 * rows] if alias else ed[2 * rows:], ng, out, 1, dpred, rows,
               cols, ldp, lde, ldp, 1.0 / n, 2.0 / n)
    got_loss, seed = out.cpu(), dpred.cpu()
    assert float(got_loss[0]) == 0.0
    d_loss = abs(float(got_loss[1] - loss64)) / float(loss64)
    assert float(seed[:, cols:].abs().max()) == 0.0, "padding columns of the seed come back zero"
    what = f"esd_head rows {rows}, ng {ng}, alias {alias}, {str(dtype)[6:]}"
    if dtype == torch.float32:
        d_seed = float((seed[:, :cols].double() - g64).abs().max()) / float(g64.abs().max())
        print(f"{what}: loss d_ref {d_ref_loss:.3e} kernel {d_loss:.3e}; seed d_ref {d_ref_seed:.3e} kernel {d_seed:.3e}")
        assert d_seed <= 4 * d_ref_seed, (d_seed, d_ref_seed)
    else:
        steps = _bf16_steps(seed[:, :cols].contiguous(), g64.to(torch.bfloat16))
        print(f"{what}: loss d_ref {d_ref_loss:.3e} kernel {d_loss:.3e}; seed within {steps} bf16 step(s) of bf16(fp64)")
        assert steps <= 1
    assert d_loss <= 4 * d_ref_loss, (d_loss, d_ref_loss)
    # loss alone (no seed) and seed alone (no accumulator)
    out2 = torch.zeros(2, device=dev, dtype=torch.float64)
    k.esd_head(predd, ed[:rows], ed[rows:2 * rows], ed[rows:2 * rows] if alias else ed[2 * rows:], ng, out2, 1, None, rows,
               cols, ldp, lde, 0, 1.0 / n, 2.0 / n)
    assert abs(float(out2[1]) - float(out[1])) <= 1e-12 * float(out[1])          # (the atomics' order is free)
    dpred2 = torch.full((rows, ldp), 3.0, device=dev, dtype=dtype)
    k.esd_head(predd, ed[:rows], ed[rows:2 * rows], ed[rows:2 * rows] if alias else ed[2 * rows:], ng, None, 0, dpred2, rows,
               cols, ldp, lde, ldp, 1.0 / n, 2.0 / n)
    assert torch.equal(dpred2, dpred)
