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


# ---------------------------------------------------------------------------------------------------------------------------
# Backward values and gradient fan-in.  A case is (HIP graph over Acts, the same graph as a torch expression over tensors and
# a dict of parameters); both return the list of outputs.  Bounds: TOL for what is GEMMs, copies and SiLU only
# (test_gemm_wgrad_linear, test_gemm_wgrad_conv, test_skinny_gemm_and_wgrad, test_elementwise_family), 2 * TOL where a
# LayerNorm / GroupNorm / GEGLU / attention backward is in the graph (test_layernorm, test_groupnorm,
# test_geglu_interleaved_layout, test_attention hold those kernels to TOL * 2).
KEYS = ("fc.weight", "fc.bias", "proj.weight", "proj.bias", "ln.weight", "ln.bias", "gn.weight", "gn.bias", "conv.weight",
        "conv.bias")


def _lnr(p, t, key="ln"):
    return F.layer_norm(t, (t.shape[1],), p[key + ".weight"], p[key + ".bias"], 1e-5)


def _gnr(p, t, silu=False):
    z = F.group_norm(t.t().reshape(1, C, M), 32, p["gn.weight"], p["gn.bias"], 1e-5)[0].t()
    return F.silu(z) if silu else z


def _linr(p, t, key, bias=True):
    y = t @ p[key + ".weight"].t()
    return y + p[key + ".bias"] if bias else y


def _geglur(pre):                  # (hidden, gate) interleaved in blocks of 8 columns
    pre = pre.view(pre.shape[0], -1, 2, 8)
    return (pre[:, :, 0] * F.gelu(pre[:, :, 1])).reshape(pre.shape[0], -1)


def _convr(p, t, mode):
    xn = t.view(1, 8, 8, 32).permute(0, 3, 1, 2)
    if mode == 2:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xn, p["conv.weight"].view(32, 3, 3, 32).permute(0, 3, 1, 2), p["conv.bias"], stride=2 if mode == 1 else 1,
                 padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, 32)


def _attn(o, qkv):
    return o.attention(qkv.t[:, :64], qkv.t[:, 64:128], qkv.t[:, 128:], 1, 1, M, M, qkv, qkv, (0, 64), ((64, 128), (128, 192)))


def _attnr(t):
    return torch.softmax(t[:, :64] @ t[:, 64:128].t() * 64 ** -0.5, -1) @ t[:, 128:]


def _rand(dev, shape, seed, dtype=torch.float32, shift=0.0):
    return (torch.randn(shape, device=dev, generator=torch.Generator(dev).manual_seed(seed)) + shift).to(dtype)


def _forward(o, hip, xs, seed=70):
    """Runs the graph with the tape on and seeds every output's gradient; returns (input Acts, seeds)."""
    from pdm.models.ops import Act
    o.train, o.tape = True, []
    o.P.grad.zero_()
    acts = [Act(x.clone()) for x in xs]
    outs = hip(o, *acts)
    seeds = [_rand(o.dev, tuple(y.t.shape), seed + i) for i, y in enumerate(outs)]
    for y, s in zip(outs, seeds):
        y.g = s.to(y.t.dtype)
    return acts, outs, seeds


def _compare(o, ref, xs, acts, seeds, keys, tol, what):
    """Input and parameter gradients of the HIP graph against fp32 autograd of `ref` (seeds: clones taken before the backward -
    a finished gradient buffer changes hands and may be summed into)."""
    torch.cuda.synchronize()
    o.train = False
    assert not o.tape
    p = {key: o.P.p(key).view(o.P.by_key[key].shape).detach().clone().requires_grad_(True) for key in keys}
    leaves = [x.float().clone().requires_grad_(True) for x in xs]
    grads = torch.autograd.grad(ref(p, *leaves), leaves + list(p.values()), [s.float() for s in seeds], allow_unused=True)
    for i, (a, gr) in enumerate(zip(acts, grads)):
        close(a.g, gr if gr is not None else torch.zeros_like(a.t), tol, f"{what}: d(input {i})")
    for key, gr in zip(p, grads[len(leaves):]):        # (a parameter the graph does not use: its gradient stays zero)
        close(o.P.g(key).view(p[key].shape), gr if gr is not None else torch.zeros_like(p[key]), tol, f"{what}: d({key})")


def _check(o, hip, ref, xs, keys, tol, what):
    acts, outs, seeds = _forward(o, hip, xs)
    seeds = [s.to(y.t.dtype).clone() for s, y in zip(seeds, outs)]
    o.backward()
    _compare(o, ref, xs, acts, seeds, keys, tol, what)


def _conv_case(mode, res, rv):
    """conv3 of the 1 x 8 x 8 x 32 image; inputs: x, then the residual [rows out, 32], then the fp32 row vector [1, 48] of which
    the conv adds columns 8..40 to every pixel."""
    def hip(o, x, *more):
        more = list(more)
        r = more.pop(0) if res else None
        return [o.conv3(x, "conv", 1, 8, 8, mode, "conv.bias", residual=r, rowvec=more[0] if rv else None,
                        rv_cols=(8, 32) if rv else None)[0]]

    def ref(p, x, *more):
        more = list(more)
        y = _convr(p, x, mode)
        if res:
            y = y + more.pop(0)
        return [y + more[0][:, 8:40] if rv else y]
    return hip, ref


OP_CASES = {
    # name: (graph, torch expression, input shapes, parameter keys, bound in units of TOL)
    "linear": (lambda o, x: [o.linear(x, "fc")], lambda p, x: [_linr(p, x, "fc", False)], ((M, C),), ("fc.weight",), 1),
    "linear bias": (lambda o, x: [o.linear(x, "fc", bias="fc.bias")], lambda p, x: [_linr(p, x, "fc")], ((M, C),),
                    ("fc.weight", "fc.bias"), 1),
    "linear ln": (lambda o, x: [o.linear(x, "fc", bias="fc.bias", ln="ln")], lambda p, x: [_linr(p, _lnr(p, x), "fc")], ((M, C),),
                  ("fc.weight", "fc.bias", "ln.weight", "ln.bias"), 2),
    "linear geglu": (lambda o, x: [o.linear(x, "proj", bias="proj.bias", geglu=True)],
                     lambda p, x: [_geglur(_linr(p, x, "proj"))], ((M, C),), ("proj.weight", "proj.bias"), 2),
    "linear residual": (lambda o, x, r: [o.linear(x, "fc", bias="fc.bias", residual=r)], lambda p, x, r: [_linr(p, x, "fc") + r],
                        ((M, C), (M, C)), ("fc.weight", "fc.bias"), 1),
    "linear out_f32": (lambda o, x: [o.linear(x, "fc", bias="fc.bias", out_f32=True)], lambda p, x: [_linr(p, x, "fc")], ((M, C),),
                       ("fc.weight", "fc.bias"), 1),
    "layernorm": (lambda o, x: [o.layernorm(x, "ln")], lambda p, x: [_lnr(p, x)], ((M, C),), ("ln.weight", "ln.bias"), 2),
    "groupnorm": (lambda o, x: [o.groupnorm(x, "gn", 1, M, 32, 2, 1e-5, False)], lambda p, x: [_gnr(p, x)], ((M, C),),
                  ("gn.weight", "gn.bias"), 2),
    "groupnorm silu": (lambda o, x: [o.groupnorm(x, "gn", 1, M, 32, 2, 1e-5, True)], lambda p, x: [_gnr(p, x, True)], ((M, C),),
                       ("gn.weight", "gn.bias"), 2),
    "geglu": (lambda o, x: [o.geglu(x)], lambda p, x: [x[:, :C // 2] * F.gelu(x[:, C // 2:])], ((M, C),), (), 2),
    "silu": (lambda o, x: [o.silu(x)], lambda p, x: [F.silu(x)], ((M, C),), (), 1),
    "concat": (lambda o, a, b: [o.concat(a, b)], lambda p, a, b: [torch.cat([a, b], 1)], ((M, 32), (M, 32)), (), 1),
    "attention": (lambda o, qkv: [_attn(o, qkv)], lambda p, t: [_attnr(t)], ((M, 192),), (), 2),
}
for _mode in (0, 1, 2):
    for _res in (False, True):
        for _rv in (False, True):
            OP_CASES[f"conv3 mode {_mode}" + " residual" * _res + " rowvec" * _rv] = _conv_case(_mode, _res, _rv) + (
                ((M, 32),) + (((64, 16, 256)[_mode], 32),) * _res + ((1, 48),) * _rv, ("conv.weight", "conv.bias"), 1)


@pytest.mark.parametrize("name", list(OP_CASES))
def test_backward_values_of_every_op_match_autograd(dev, ops, name):
    """Every op on the default fp32 Ops: the input gradients and every parameter gradient against fp32 autograd of the torch
    expression test_every_op_matches_torch_fp32 compares the forward with."""
    hip, ref, shapes, keys, mult = OP_CASES[name]
    xs = [_rand(dev, shape, 100 + i, shift=0.0 if name == "attention" else 0.3) for i, shape in enumerate(shapes)]
    _check(ops, hip, ref, xs, keys, TOL["f32"] * mult, name)


def test_backward_values_of_the_skinny_linear_match_autograd(dev, ops):
    """M = 8 rows: the weight-streaming forward, pdmk_skinny_wgrad and the skinny input gradient."""
    xs = [_rand(dev, (8, C), 110, shift=0.3)]
    _check(ops, lambda o, x: [o.linear(x, "fc", bias="fc.bias")], lambda p, x: [_linr(p, x, "fc")], xs, ("fc.weight", "fc.bias"),
           TOL["f32"], "skinny linear")


# Fan-in graphs: every way a second gradient meets the slot of `x` (pdm.models.ops.Act).  Ops registered LATER run EARLIER in the
# backward pass.  Inputs are [64, 64]; the first is the shared tensor x.
FANIN = {
    # two writers: the second accumulates into the buffer the first one wrote (owned)
    "two linears": (lambda o, x: [o.linear(x, "fc"), o.linear(x, "proj")],
                    lambda p, x: [_linr(p, x, "fc", False), _linr(p, x, "proj", False)], 1, 1),
    # the residual's finished gradient is taken over, the LayerNorm / GroupNorm backward accumulates into it
    "ln residual": (lambda o, x: [o.linear(o.layernorm(x, "ln"), "fc", residual=x)],
                    lambda p, x: [_linr(p, _lnr(p, x), "fc", False) + x], 1, 2),
    "gn residual": (lambda o, x: [o.linear(o.groupnorm(x, "gn", 1, M, 32, 2, 1e-5, False), "fc", residual=x)],
                    lambda p, x: [_linr(p, _gnr(p, x), "fc", False) + x], 1, 2),
    # a writer first, so the residual's gradient waits as the pending addend (defer_fanin) and the norm's store absorbs it
    "ln residual after a writer": (lambda o, x: [o.linear(o.layernorm(x, "ln"), "fc", residual=x), o.linear(x, "proj")],
                                   lambda p, x: [_linr(p, _lnr(p, x), "fc", False) + x, _linr(p, x, "proj", False)], 1, 2),
    "gn residual after a writer": (lambda o, x: [o.linear(o.groupnorm(x, "gn", 1, M, 32, 2, 1e-5, False), "fc", residual=x),
                                                 o.linear(x, "proj")],
                                   lambda p, x: [_linr(p, _gnr(p, x), "fc", False) + x, _linr(p, x, "proj", False)], 1, 2),
    # a writer without an addend port, then the finished gradient: added on the next read
    "residual then linear": (lambda o, x, u: [o.linear(u, "fc", residual=x), o.linear(x, "proj")],
                             lambda p, x, u: [_linr(p, u, "fc", False) + x, _linr(p, x, "proj", False)], 2, 1),
    # a writer, the finished gradient as the pending addend (defer_fanin), then a second writer without an addend port: it adds
    # the pending one before it accumulates
    "linear, residual, linear": (lambda o, x, u: [o.linear(x, "proj"), o.linear(u, "fc", residual=x), o.linear(x, "fc")],
                                 lambda p, x, u: [_linr(p, x, "proj", False), _linr(p, u, "fc", False) + x, _linr(p, x, "fc", False)],
                                 2, 1),
    # an aliased view of the concat's gradient, then a writer accumulates into the view
    "concat then linear": (lambda o, x, b: [o.linear(x, "fc"), o.concat(x, b)],
                           lambda p, x, b: [_linr(p, x, "fc", False), torch.cat([x, b], 1)], 2, 1),
    # two finished gradients, no writer
    "two residuals": (lambda o, x, u, v: [o.linear(u, "fc", residual=x), o.linear(v, "proj", residual=x)],
                      lambda p, x, u, v: [_linr(p, u, "fc", False) + x, _linr(p, v, "proj", False) + x], 3, 1),
}
FKEYS = ("fc.weight", "proj.weight", "ln.weight", "ln.bias", "gn.weight", "gn.bias")


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("name", list(FANIN))
def test_gradient_fan_in_matches_autograd(dev, ops, name, defer):
    hip, ref, nin, mult = FANIN[name]
    xs = [_rand(dev, (M, C), 120 + i, shift=0.3) for i in range(nin)]
    ops.defer_fanin = defer
    try:
        _check(ops, hip, ref, xs, FKEYS, TOL["f32"] * mult, f"{name} defer={defer}")
    finally:
        ops.defer_fanin = False


# What arrives at x while its gradient slot holds a LENT buffer: the graph registered before `linear(u, "fc", residual=x)`, which
# therefore runs after that Linear's backward has parked its dy on x.  ("read first": .g is read before the writer runs.)
LENT = {
    "writer": (lambda o, x: [o.linear(x, "proj")], lambda p, x: [_linr(p, x, "proj", False)], 0, 1),
    "read first, then writer": (lambda o, x: [o.linear(x, "proj")], lambda p, x: [_linr(p, x, "proj", False)], 0, 1),
    "layernorm": (lambda o, x: [o.linear(o.layernorm(x, "ln"), "proj")], lambda p, x: [_linr(p, _lnr(p, x), "proj", False)], 0, 2),
    "groupnorm": (lambda o, x: [o.linear(o.groupnorm(x, "gn", 1, M, 32, 2, 1e-5, False), "proj")],
                  lambda p, x: [_linr(p, _gnr(p, x), "proj", False)], 0, 2),
    "concat view": (lambda o, x, b: [o.concat(x, b)], lambda p, x, b: [torch.cat([x, b], 1)], 1, 1),
    "second residual": (lambda o, x, v: [o.linear(v, "proj", residual=x)], lambda p, x, v: [_linr(p, v, "proj", False) + x], 1, 1),
    "read first, then second residual": (lambda o, x, v: [o.linear(v, "proj", residual=x)],
                                         lambda p, x, v: [_linr(p, v, "proj", False) + x], 1, 1),
}


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("name", list(LENT))
def test_lent_gradient_buffer_is_never_written(dev, ops, name, defer):
    """Weight gradients are being collected (Ops._wg_open, the hook the U-Net engine puts around a transformer block), so the dy of
    `linear(u, "fc", residual=x)` is parked on x while the deferred weight gradient still reads it.  Whatever arrives at x next
    must leave that buffer bit-identical until flush_pending() has issued the weight gradient; afterwards the collected weight and
    bias gradients and x.g match autograd.  The "read first" orders - x.g is read, which hands out the lent buffer, and only then
    a gradient accumulates - are the ones the code before the gradient slot got wrong with defer_fanin False: the read made the
    lent buffer the Act's own and the accumulate went into it in place."""
    first, ref_first, nmore, mult = LENT[name]
    xs = [_rand(dev, (M, C), 140 + i, shift=0.3) for i in range(2 + nmore)]          # x, u, then the inputs of `first`
    snap = []

    def hip(o, x, u, *more):
        outs = first(o, x, *more)
        if name.startswith("read first"):
            o.tape.append(lambda: x.g)
        o.tape.append(lambda: snap.append((parked.g, parked.g.clone())))       # runs right after the Linear below parked its dy
        parked = o.linear(u, "fc", bias="fc.bias", residual=x)
        return outs + [parked]

    def ref(p, x, u, *more):
        return ref_first(p, x, *more) + [_linr(p, u, "fc") + x]

    o = ops
    o.defer_fanin = defer
    try:
        acts, outs, seeds = _forward(o, hip, xs)
        seeds = [s.clone() for s in seeds]
        tape, o.tape = o.tape, []
        o._wg_open()
        for fn in reversed(tape):
            fn()
        torch.cuda.synchronize()
        (dy, dy0), = snap
        assert dy is outs[-1].g and torch.equal(dy, dy0), "the lent buffer was written before the weight gradient that reads it ran"
        o.flush_pending()
        _compare(o, ref, xs, acts, seeds, FKEYS + ("fc.bias",), TOL["f32"] * mult, f"lent, {name}, defer={defer}")
    finally:
        o.defer_fanin = False
        o._wg_flush()


# ---------------------------------------------------------------------------------------------------------------------------
# The fused forms of Linear, which only the bf16 training configuration takes.
@pytest.fixture(scope="module")
def ops_bf16(dev):
    from pdm import _pdmk as k
    from pdm.models.ops import Ops
    from pdm.models.unet.params import ParamStore, _lin, _vec, assign_offsets, norm_pair
    entries = assign_offsets([_lin("fc", [("fc.weight", C)], C), _vec("fc.bias", [("fc.bias", C)]),
                              _lin("proj", [("proj.weight", C)], C), _vec("proj.bias", [("proj.bias", C)]),
                              _lin("down", [("down.weight", C)], C // 2), _vec("down.bias", [("down.bias", C)]),
                              *norm_pair("ln", C)])
    store = ParamStore(entries, dev, torch.bfloat16, train=True)
    g = torch.Generator(dev).manual_seed(13)
    for e in entries:
        v = store.p(e.key)
        if e.kind == "vec":
            v.copy_(torch.randn(e.numel, device=dev, generator=g) * 0.3 + (e.key == "ln.weight"))
        else:
            v.copy_(torch.randn(e.numel, device=dev, generator=g) * (e.numel // e.shape[0]) ** -0.5)
    store.refresh()
    return Ops(store, torch.bfloat16, fuse_geglu=True, fuse_ln=2, fuse_geglu_bwd=True, defer_fanin=True, partials=k.PartialQueue(),
               slabs=k.SlabQueue(), group_wgrad=True)


BF16_FORMS = {
    # name: (graph, torch expression, parameter keys, launch wrappers that must NOT run, LayerNorm prologue expected)
    "ln": (lambda o, x: [o.linear(x, "fc", bias="fc.bias", ln="ln")], lambda p, x: [_linr(p, _lnr(p, x), "fc")],
           ("fc.weight", "fc.bias", "ln.weight", "ln.bias"), ("layernorm_fwd",), True),
    "ln geglu": (lambda o, x: [o.linear(x, "proj", bias="proj.bias", geglu=True, ln="ln")],
                 lambda p, x: [_geglur(_linr(p, _lnr(p, x), "proj"))], ("proj.weight", "proj.bias", "ln.weight", "ln.bias"),
                 ("layernorm_fwd", "geglu_fwd"), True),
    "geglu": (lambda o, x: [o.linear(x, "proj", bias="proj.bias", geglu=True)], lambda p, x: [_geglur(_linr(p, x, "proj"))],
              ("proj.weight", "proj.bias"), ("geglu_fwd",), False),
    "geglu -> linear": (lambda o, x: [o.linear(o.linear(x, "proj", bias="proj.bias", geglu=True), "down", bias="down.bias")],
                        lambda p, x: [_linr(p, _geglur(_linr(p, x, "proj")), "down")],
                        ("proj.weight", "proj.bias", "down.weight", "down.bias"), ("geglu_fwd", "geglu_bwd"), False),
}


@pytest.mark.parametrize("name", list(BF16_FORMS))
def test_fused_linear_forms_at_bf16_match_fp32_torch(dev, ops_bf16, monkeypatch, name):
    """The LayerNorm prologue, the fused GEGLU epilogue (with and without the prologue) and the fused GEGLU backward of the
    consuming Linear at [64, 64] in bf16: forward and backward against fp32 torch on the fp32 master parameters, 2 * TOL as every
    graph here has a LayerNorm or GEGLU backward in it (test_layernorm, test_geglu_interleaved_layout).  The fused form must
    really be taken: the stand-alone kernel it replaces is never launched, and the prologue runs in the row-block kernel."""
    from pdm import _pdmk as k
    hip, ref, keys, banned, rowblock = BF16_FORMS[name]
    o, calls = ops_bf16, []
    for fn in ("layernorm_fwd", "geglu_fwd", "geglu_bwd"):
        monkeypatch.setattr(k, fn, lambda *a, _n=fn, _f=getattr(k, fn), **kw: (calls.append(_n), _f(*a, **kw))[1])
    x = _rand(dev, (M, C), 160, torch.bfloat16, shift=0.3)
    acts, outs, seeds = _forward(o, hip, [x])
    if rowblock:
        assert "rowblock_kernel" in k.candidate_name(k.A_ROWK, k.B_ROWK, k.last_candidate())
    p = {key: o.P.p(key).view(o.P.by_key[key].shape) for key in keys}
    close(outs[0].t, ref(p, x.float())[0], TOL["bf16"], f"{name}: forward")
    seeds = [s.to(torch.bfloat16).clone() for s in seeds]
    o.backward()
    _compare(o, ref, [x], acts, seeds, keys, TOL["bf16"] * 2, name)
    assert not [c for c in calls if c in banned], calls
