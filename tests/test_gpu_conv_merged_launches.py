"""The fp32 conv stage launches kernels of one layer call that do not depend on each other together: the weight transform inside the input transform's
launch (forward, and a data gradient that has to transform the weights itself), and -- behind frcnn_conv3x3_f32_bwd -- the data gradient's output
transform with the weight gradient's last kernel.  Every element keeps its instruction sequence, so every output must keep its BITS: the shared
launches (the default) are compared with the separate ones, which the library keeps under its profiler brackets (_lib.prof_enable(True)), and the
one-call backward with the two calls it stands for.  torch.equal everywhere; no tolerance."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def T():
    from faster_rcnn_pytorch_amd import _lib, ops
    return ops, _lib


@contextlib.contextmanager
def _zeroed_buffers():
    """Output buffers zero-filled instead of uninitialised: the sign words and the transforms have padding entries that no kernel writes or reads."""
    empty = torch.empty
    torch.empty = torch.zeros
    try:
        yield
    finally:
        torch.empty = empty


@contextlib.contextmanager
def _separate_launches(_lib, on):
    _lib.prof_enable(bool(on))
    try:
        yield
    finally:
        _lib.prof_enable(False)
        if on:
            _lib.prof_report()                                        # retire the brackets' events
            _lib.prof_reset()


def _tile(ops, hw):
    from faster_rcnn_pytorch_amd.ops import _host_i32, _np_ptr, lib
    H, W = _host_i32([h for h, _ in hw]), _host_i32([w for _, w in hw])
    return int(lib.frcnn_conv3x3_f32_tile_size(_np_ptr(H), _np_ptr(W), len(hw)))


def _layer(Cin, Cout, hw, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    xs = [torch.randn(1, Cin, h, wd, generator=g).to(DEV) for h, wd in hw]
    return w, b, xs, g


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert (p is None) == (q is None), (what, i)
        if p is not None:
            assert p.dtype == q.dtype and p.shape == q.shape and torch.equal(p, q), (what, i)


# ---------------------------------------------------------------------------------------------------------------- forward: weight || input
def _forward(ops, w, b, xs, relu, pool):
    with _zeroed_buffers():
        urot = ops.conv3x3_u_buffer(xs, w)
        ys, xt, bits = ops.conv3x3_fwd(xs, w, b, relu, keep_transformed=True, want_bits=relu, pool=pool, u_rotated=urot)
        plain = ops.conv3x3_fwd(xs, w, b, relu, pool=pool)              # no rotated transform: the weight blocks are half as many
    torch.cuda.synchronize()
    return [*ys, xt, bits, urot, *plain]


FWD_LAYERS = {                                                          # name: (Cin, Cout, levels, tile)
    "64-128_40x52": (64, 128, [(40, 52)], 4),
    "512-512_8x12": (512, 512, [(8, 12)], 2),                          # 2048 weight blocks beside ONE strip per channel: the weight rows stride
    "64-64_two_levels": (64, 64, [(24, 32), (12, 16)], 2),             # strips of two levels in one grid row
    "128-128_two_levels": (128, 128, [(24, 32), (12, 16)], 2),
}


@pytest.mark.parametrize("act", ["none", "relu", "pool"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("name", list(FWD_LAYERS))
def test_forward_with_the_weight_transform_in_the_input_launch_keeps_every_bit(T, name, bias, act):
    ops, _lib = T
    Cin, Cout, hw, m = FWD_LAYERS[name]
    assert _tile(ops, hw) == m
    if act == "pool" and m != 4:
        act = "relu"                                                    # the fused pooling lives in the 4 x 4 tile; the 2 x 2 layer repeats its ReLU case
    w, b, xs, _ = _layer(Cin, Cout, hw, 11)
    b = b if bias else None
    with _separate_launches(_lib, True):
        ref = _forward(ops, w, b, xs, act != "none", act == "pool")
    with _separate_launches(_lib, False):
        got = _forward(ops, w, b, xs, act != "none", act == "pool")
        again = _forward(ops, w, b, xs, act != "none", act == "pool")
    _same(got, ref, "shared launch vs separate launches")
    _same(again, got, "run twice")
    y64 = torch.nn.functional.conv2d(xs[0].double(), w.double(), None if b is None else b.double(), padding=1)      # (and it is still the convolution)
    if act != "none":
        y64 = torch.relu(y64)
    if act == "pool":
        y64 = torch.nn.functional.max_pool2d(y64, 2, 2)
    assert float((got[0].double() - y64).abs().max()) < 1e-4 * max(1.0, float(y64.abs().max()))


def test_the_separate_form_is_separate_and_the_shared_form_is_shared(T):
    """What the two forms launch, by the library's own per-kernel brackets: with them on, a forward is weight + input + product + output; the
    shared launch carries a name of its own, which the brackets therefore never see."""
    ops, _lib = T
    w, b, xs, _ = _layer(64, 128, [(40, 52)], 3)
    _lib.prof_report()
    _lib.prof_reset()
    with _separate_launches(_lib, True):
        ops.conv3x3_fwd(xs, w, b, True)
        torch.cuda.synchronize()
        rep = _lib.prof_report()
        assert {k: n for k, (_, n) in rep.items()} == {"rpn_wino_weight_kernel": 1, "rpn_wino_input_kernel": 1, "rpn_wino_gemm_kernel": 1, "rpn_wino_output_kernel": 1}


# ---------------------------------------------------------------------------------------------------------------- backward: one call per layer
def _backward(ops, w, b, xs, gs, act, bias, how):
    """Forward as the training step makes it, then both gradients: how = 'two' (bwd_data + wgrad, the calls the one-call form stands for) or 'one'."""
    relu, pool = act != "none", act == "pool"
    hw = [tuple(x.shape[2:]) for x in xs]
    with _zeroed_buffers():
        urot = ops.conv3x3_u_buffer(xs, w)
        ys, xt, bits = ops.conv3x3_fwd(xs, w, b if bias else None, relu, keep_transformed=True, want_bits=relu, pool=pool, u_rotated=urot)
        if how == "one":
            dxs, dw, db = ops.conv3x3_bwd(gs, w, xt, bits, hw if pool else None, u_rotated=urot, want_bias=bias)
        else:
            dyt = ops.conv3x3_dy_buffer(hw, int(w.shape[0]), DEV)
            dxs = ops.conv3x3_bwd_data(gs, w, bits, hw if pool else None, u_rotated=urot, dy_transformed=dyt, want_bias_partials=bias)
            dw, db = ops.conv3x3_wgrad(xs, gs, bits, want_bias=bias, x_transformed=xt, pooled=pool, dy_transformed=dyt)
    torch.cuda.synchronize()
    return [*dxs, dw, db]


BWD_LAYERS = {                                                          # one shape per scheduling mode of the data gradient's product (wn_run's rules)
    "many_64-128_244x244": (64, 128, (244, 244)),                      # 3721 output tiles = 36 planes x 1 x 30 product tiles on 512 workgroup slots (2.1 each: the
                                                                        # rounding to whole tiles would cost 42 %, so these ranges still cut tiles)
    "whole_128-128_276x276": (128, 128, (276, 276)),                   # 36 x 1 x 38 = 1368 tiles, 3 per slot within 16 %: ranges cut at tile boundaries
    "streamk_256-256_40x52": (256, 256, (40, 52)),                     # 216 tiles on 512 slots: stream-K with partial tiles, slabs and tickets
    "onetile_512-512_37x62": (512, 512, (37, 62)),                     # 432 tiles >= 3/4 of the slots: one whole tile per workgroup
}


@pytest.mark.parametrize("products", ["native", "split"])
@pytest.mark.parametrize("act,bias", [("none", False), ("relu", True), ("pool", True), ("pool", False)])
@pytest.mark.parametrize("name", list(BWD_LAYERS))
def test_one_call_backward_keeps_every_bit_of_the_two_calls(T, name, act, bias, products):
    ops, _lib = T
    Cin, Cout, (h, wd) = BWD_LAYERS[name]
    assert _tile(ops, [(h, wd)]) == 4
    w, b, xs, g = _layer(Cin, Cout, [(h, wd)], 23)
    gs = [torch.randn(1, Cout, h // 2 if act == "pool" else h, wd // 2 if act == "pool" else wd, generator=g).to(DEV)]
    ops.conv3x3_f32_products(products)
    try:
        with _separate_launches(_lib, False):
            two = _backward(ops, w, b, xs, gs, act, bias, "two")
            one = _backward(ops, w, b, xs, gs, act, bias, "one")
            again = _backward(ops, w, b, xs, gs, act, bias, "one")
        with _separate_launches(_lib, True):
            apart = _backward(ops, w, b, xs, gs, act, bias, "one")
    finally:
        ops.conv3x3_f32_products("native")
    _same(one, two, "one call vs bwd_data + wgrad")
    _same(again, one, "run twice")
    _same(apart, one, "separate launches vs the shared one")
    assert (one[-1] is not None) == bias


def test_fallbacks_equal_the_calls_they_keep(T):
    """One gradient only, or no cached transform: the autograd function and the plain calls keep today's launches, whose weight transform may now ride in
    the input transform's launch (a data gradient without the forward's rotated weights)."""
    ops, _lib = T
    Cin, Cout, h, wd = 128, 128, 40, 52
    w, b, xs, g = _layer(Cin, Cout, [(h, wd)], 31)
    x = xs[0]
    gy = torch.randn(1, Cout, h, wd, generator=g).to(DEV)

    def plain_calls():
        with _zeroed_buffers():
            ys, _, bits = ops.conv3x3_fwd([x], w, b, True, want_bits=True)
            dx = ops.conv3x3_bwd_data([gy], w, bits)[0]                 # transforms the weights itself; nothing cached
            dw, db = ops.conv3x3_wgrad([x], [gy], bits, want_bias=True)     # transforms x and the gradient itself
        torch.cuda.synchronize()
        return [ys[0], dx, dw, db]

    with _separate_launches(_lib, True):
        ref = plain_calls()
    with _separate_launches(_lib, False):
        got = plain_calls()
    _same(got, ref, "no cached transform")
    y_ref, dx_ref, dw_ref, db_ref = ref

    def autograd(need_x, need_w):
        xi = x.clone().requires_grad_(need_x)
        wi, bi = w.clone().requires_grad_(need_w), b.clone().requires_grad_(need_w)
        y = ops.conv3x3(xi, wi, bi, relu=True)
        y.backward(gy)
        torch.cuda.synchronize()
        return y.detach(), xi.grad, wi.grad, bi.grad

    for need_x, need_w in ((True, False), (False, True), (True, True)):     # only dx; only dw (+ db); both: the one-call form
        y, dx, dw, db = autograd(need_x, need_w)
        assert torch.equal(y, y_ref)
        assert (dx is None) == (not need_x) and (dw is None) == (not need_w) and (db is None) == (not need_w)
        if need_x:
            assert torch.equal(dx, dx_ref)
        if need_w:
            assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)


def test_forward_and_backward_captured_twice_from_one_pool_equal_eager(T):
    """A layer's forward + backward (the shared launches and the one-call backward) captured into two HIP graphs that share one memory pool, each replayed
    twice: the bits of the eager step."""
    ops, _lib = T
    layers = [(64, 128, 40, 52, True), (256, 256, 40, 52, False)]
    eager, inputs = [], []
    for Cin, Cout, h, wd, pool in layers:
        w, b, xs, g = _layer(Cin, Cout, [(h, wd)], 41)
        gy = torch.randn(1, Cout, h // 2 if pool else h, wd // 2 if pool else wd, generator=g).to(DEV)
        x = xs[0].requires_grad_(True)
        w.requires_grad_(True)
        b.requires_grad_(True)
        inputs.append((x, w, b, gy, pool))
        y = ops.conv3x3(x, w, b, relu=True, pool=pool)
        eager.append([y.detach().clone()] + [t.clone() for t in torch.autograd.grad(y, (x, w, b), gy)])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                                          # warm-up on a side stream, as torch asks before a capture
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for x, w, b, gy, pool in inputs:
            torch.autograd.grad(ops.conv3x3(x, w, b, relu=True, pool=pool), (x, w, b), gy)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphs, outs, pool_id = [], [], None
    for x, w, b, gy, pool in inputs:
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, pool=pool_id):
            y = ops.conv3x3(x, w, b, relu=True, pool=pool)
            outs.append([y.detach()] + list(torch.autograd.grad(y, (x, w, b), gy)))
        pool_id = gr.pool()
        graphs.append(gr)
    for _ in range(2):
        for gr in graphs:
            gr.replay()
    torch.cuda.synchronize()
    for got, ref in zip(outs, eager):
        _same(got, ref, "graph replay vs eager")
