"""Every op of `pdm.models.ops.Ops` runs on a default-constructed `Ops(store, dtype)` - the object the VAE and both CLIP towers
build - and computes what torch computes in fp32 (-m gpu).  The store is a throw-away arena filled with random numbers.
Tolerances are the ones tests/test_kernels_gpu.py applies to the kernel behind each op in fp32 (its `close` and `TOL`)."""
import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import TOL, close

pytestmark = pytest.mark.gpu

M, C = 64, 64            # activations [64, 64]; the image of the convs is 1 x 8 x 8 x 32


@pytest.fixture(scope="module")
def ops(dev):
    from pdm.models.ops import Ops
    from pdm.models.unet.params import ParamStore, _conv, _lin, _vec, assign_offsets, norm_pair
    entries = assign_offsets([_lin("fc", [("fc.weight", C)], C), _vec("fc.bias", [("fc.bias", C)]),
                              _lin("proj", [("proj.weight", C)], C), _vec("proj.bias", [("proj.bias", C)]),
                              *norm_pair("ln", C), *norm_pair("gn", C),
                              _conv("conv", 32, 32), _vec("conv.bias", [("conv.bias", 32)])])
    store = ParamStore(entries, dev, torch.float32, train=True)
    g = torch.Generator(dev).manual_seed(11)
    for e in entries:
        v = store.p(e.key)
        if e.kind == "vec":
            v.copy_(torch.randn(e.numel, device=dev, generator=g) * 0.3 + (e.key in ("ln.weight", "gn.weight")))
        else:
            v.copy_(torch.randn(e.numel, device=dev, generator=g) * (e.numel // e.shape[0]) ** -0.5)
    store.refresh()
    return Ops(store, torch.float32)


def _x(dev, seed, cols=C, shift=0.3):
    return torch.randn(M, cols, device=dev, generator=torch.Generator(dev).manual_seed(seed)) + shift


def _w(o, key):
    return o.P.p(key).view(o.P.by_key[key].shape)


def _conv_ref(o, x, mode):
    xn = x.view(1, 8, 8, 32).permute(0, 3, 1, 2)
    if mode == 2:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xn, _w(o, "conv.weight").view(32, 3, 3, 32).permute(0, 3, 1, 2), o.P.p("conv.bias"),
                 stride=2 if mode == 1 else 1, padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, 32)


def test_every_op_matches_torch_fp32(dev, ops):
    from pdm.models.ops import Act
    o, tol = ops, TOL["f32"]
    o.train, o.tape = False, []
    ln = lambda t: F.layer_norm(t, (C,), o.P.p("ln.weight"), o.P.p("ln.bias"), 1e-5)
    x = _x(dev, 1)
    close(o.layernorm(Act(x), "ln").t, ln(x), tol, "layernorm")                                     # test_layernorm
    close(o.linear(Act(x), "fc", bias="fc.bias", ln="ln").t, ln(x) @ _w(o, "fc.weight").t() + o.P.p("fc.bias"), tol,
          "linear(ln=)")                                                                            # test_gemm_linear
    pre = (x @ _w(o, "proj.weight").t() + o.P.p("proj.bias")).view(M, C // 16, 2, 8)                # rows (hidden, gate)-interleaved by 8
    close(o.linear(Act(x), "proj", bias="proj.bias", geglu=True).t, (pre[:, :, 0] * F.gelu(pre[:, :, 1])).reshape(M, C // 2), tol,
          "linear(geglu=True)")                                                                     # test_geglu_interleaved_layout
    close(o.geglu(Act(x)).t, x[:, :C // 2] * F.gelu(x[:, C // 2:]), tol, "geglu")                   # test_elementwise_family
    close(o.silu(Act(x)).t, F.silu(x), tol, "silu")                                                 # test_elementwise_family
    for silu in (False, True):                                                                      # test_groupnorm
        z = F.group_norm(x.t().reshape(1, C, M), 32, o.P.p("gn.weight"), o.P.p("gn.bias"), 1e-5)
        close(o.groupnorm(Act(x), "gn", 1, M, 32, 2, 1e-5, silu).t, (F.silu(z) if silu else z)[0].t(), tol, f"groupnorm silu={silu}")
    xi = _x(dev, 2, 32)
    for mode, side in ((0, 8), (1, 4), (2, 16)):                                                    # test_gemm_conv_fwd_modes
        y, Ho, Wo = o.conv3(Act(xi), "conv", 1, 8, 8, mode, "conv.bias")
        assert (Ho, Wo) == (side, side)
        close(y.t, _conv_ref(o, xi, mode), tol, f"conv3 mode {mode}")
    a, b = _x(dev, 3, 32), _x(dev, 4, 32)
    assert torch.equal(o.concat(Act(a), Act(b)).t, torch.cat([a, b], 1))                            # test_elementwise_family (copy2d)
    qkv = Act(_x(dev, 5, 192, 0.0))
    att = o.attention(qkv.t[:, :64], qkv.t[:, 64:128], qkv.t[:, 128:], 1, 1, M, M, qkv, qkv, (0, 64), ((64, 128), (128, 192)))
    q, kk, v = qkv.t[:, :64], qkv.t[:, 64:128], qkv.t[:, 128:]
    close(att.t, torch.softmax(q @ kk.t() * 64 ** -0.5, -1) @ v, tol, "attention")                  # test_attention


def test_backward_and_flush_on_a_default_ops(dev, ops):
    """train=True on the same object: every op's backward closure and flush_pending() run without the U-Net engine's
    training queues, and every gradient they leave is finite."""
    from pdm.models.ops import Act
    o = ops
    o.train, o.tape = True, []
    o.P.grad.zero_()
    ins = [Act(_x(dev, 20 + i)) for i in range(6)]
    outs = [o.linear(ins[0], "fc", bias="fc.bias", ln="ln"), o.layernorm(ins[1], "ln"),
            o.linear(ins[2], "proj", bias="proj.bias", geglu=True), o.geglu(ins[3]), o.silu(ins[4]),
            o.groupnorm(ins[5], "gn", 1, M, 32, 2, 1e-5, True)]
    for mode in (0, 1, 2):
        ins.append(Act(_x(dev, 30 + mode, 32)))
        outs.append(o.conv3(ins[-1], "conv", 1, 8, 8, mode, "conv.bias")[0])
    ins += [Act(_x(dev, 40, 32)), Act(_x(dev, 41, 32)), Act(_x(dev, 42, 192, 0.0))]
    qkv = ins[-1]
    outs += [o.concat(ins[-3], ins[-2]),
             o.attention(qkv.t[:, :64], qkv.t[:, 64:128], qkv.t[:, 128:], 1, 1, M, M, qkv, qkv, (0, 64), ((64, 128), (128, 192)))]
    for i, y in enumerate(outs):
        y.g = torch.randn(y.t.shape, device=dev, generator=torch.Generator(dev).manual_seed(50 + i))
    o.backward()
    o.flush_pending()
    torch.cuda.synchronize()
    o.train = False
    assert not o.tape
    for i, a in enumerate(ins):
        assert a.g is not None and a.g.shape == a.t.shape and torch.isfinite(a.g).all(), f"input gradient {i}"
    assert torch.isfinite(o.P.grad).all()
    for key in ("fc.weight", "fc.bias", "proj.weight", "proj.bias", "ln.weight", "ln.bias", "gn.weight", "gn.bias", "conv.weight",
                "conv.bias"):
        assert o.P.g(key).abs().max().item() > 0, f"no gradient reached {key}"
