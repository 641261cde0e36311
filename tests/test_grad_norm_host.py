"""CPU-only checks of the device-side gradient norm and clipping (csrc/grad_norm.hip, optim.DeviceSGD(max_grad_norm=, skip_nonfinite=)):

  * the numpy restatement of the documented summation order (tests/grad_norm_ref.py) against an exact sum -- Python integers on exact
    data, math.fsum of the exact squares otherwise -- within D * 2^-53 relative, D the number of additions on the longest path,
    computed from (numel, n_chunks, T), not fitted;
  * the clipped update: g.mul_(coef) then torch.optim.SGD.step() on the CPU equals tests/sgd_ref.py on the scaled gradients, bit for bit;
  * norm, coefficient, skip word and counters of the restatement on values whose answer is known;
  * the C ABI's refusals and workspace sizes, and DeviceSGD's refusals of a bad max_grad_norm / norm type, with no device touched."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import grad_norm_ref as gn
import sgd_ref

LENS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 16385]


def _within(value, exact, D):
    """|value - exact| <= D * 2^-53 * exact, in exact rational arithmetic."""
    return abs(Fraction(float(value)) - exact) * 2 ** 53 <= D * exact


def test_restatement_is_exact_on_exact_data():
    """Integers times a power of two, sum of squares below 2^53 units: every partial sum is an integer below 2^53 units and every
    addition is exact, in any order."""
    rs = np.random.RandomState(0)
    for scale in (1.0, 2.0 ** -20, 2.0 ** 30):
        ints = [rs.randint(-300, 301, n).astype(np.int64) for n in LENS + [1000003 // 8]]
        exact = sum(int(v) * int(v) for t in ints for v in t)
        assert 0 < exact < 2 ** 53
        got, bad = gn.sumsq_of([(t * scale).astype(np.float32) for t in ints])
        assert bad == 0 and Fraction(float(got)) == exact * Fraction(scale) ** 2, scale


@pytest.mark.parametrize("T", [gn.FINISH_THREADS, 64])
def test_restatement_is_within_the_bound_of_its_longest_path(T):
    rs = np.random.RandomState(1)
    for lens, sigma in ((LENS, 0.02), ([1] * (2 * T + 1), 1.0), ([40000, 7], 1e-20), ([3 * gn.CHUNK + 5], 3e18)):
        ts = [(rs.standard_normal(n) * sigma).astype(np.float32) for n in lens]
        D = gn.additions_on_the_longest_path(lens, T)
        exact = Fraction(math.fsum(float(np.float64(v) * np.float64(v)) for t in ts for v in t))
        got, bad = gn.sumsq_of(ts, T)
        assert bad == 0 and exact > 0 and _within(got, exact, D), (lens[:4], sigma, D, float(got), float(exact))
    # D itself, on sizes where it can be counted by hand: one chunk of 5 elements -> 1 + 2 + 6 + 3; one trip -> 1 + 6 + (T / 64 - 1)
    assert gn.additions_on_the_longest_path([5], T) == 12 + 1 + 6 + T // 64 - 1
    assert gn.additions_on_the_longest_path([gn.CHUNK] * (T + 1), T) == 8 + 11 + 2 + 6 + T // 64 - 1
    assert gn.additions_on_the_longest_path([1025, 0], T) == 2 + 11 + 1 + 6 + T // 64 - 1


def test_order_depends_on_position_only():
    """A tensor's contribution is that of its chunks; a chunk's partial is that of the chunk alone."""
    rs = np.random.RandomState(2)
    x = rs.standard_normal(2 * gn.CHUNK + 77).astype(np.float32)
    p, c = gn.chunk_partials(x)
    for k in range(3):
        q, _ = gn.chunk_partials(x[k * gn.CHUNK:(k + 1) * gn.CHUNK])
        assert p[k].tobytes() == q[0].tobytes()
    assert len(p) == 3 and c.tolist() == [0, 0, 0]
    # thread 0's first accumulator holds elements 0 and 1024: three values whose sum depends on the order show which one is used
    y = np.zeros(gn.CHUNK, np.float32)
    y[0], y[1024], y[4] = 2.0 ** 30, 2.0 ** 3, 2.0 ** 3                  # squares 2^60, 2^6, 2^6: (2^60 + 2^6) + 2^6 != 2^60 + (2^6 + 2^6)
    y[2048] = 2.0 ** 3
    got = gn.chunk_partials(y)[0][0]
    a0 = (np.float64(2.0 ** 60) + 2.0 ** 6) + 2.0 ** 6                      # element 0, 1024, 2048 in that order: thread 0, accumulator 0
    assert got == a0 + np.float64(2.0 ** 6)                                # element 4 belongs to thread 1: joins in the butterfly


def test_norm_coef_skip_and_counters():
    one = [np.array([3.0, 4.0], np.float32)]
    s = gn.state_after(one, 1.0, gn.CLIP)
    assert s["sumsq"] == 25.0 and s["norm"] == 5.0 and s["coef"] == np.float32(1.0) / (np.float32(5.0) + np.float32(1e-6)) and s["skip"] == 0
    assert gn.state_after(one, 10.0, gn.CLIP)["coef"] == 1.0 and gn.state_after(one, 1.0, 0)["coef"] == 1.0
    zero = gn.state_after([np.zeros(9, np.float32), -np.zeros(5, np.float32)], 0.5, gn.CLIP)
    assert zero["norm"] == 0.0 and zero["coef"] == 1.0 and gn.f64_bits(zero["sumsq"]) == 0
    huge = gn.state_after([np.full(70000, 3e38, np.float32)], 1.0, gn.CLIP | gn.SKIP_NONFINITE)
    assert np.isfinite(huge["sumsq"]) and np.isinf(huge["norm"]) and huge["coef"] == 0.0 and huge["skip"] == 0 and huge["nonfinite"] == 0
    tiny = gn.state_after([np.full(100, 1e-42, np.float32)], 1.0, gn.CLIP)
    assert tiny["sumsq"] > 0 and tiny["coef"] == 1.0
    for bad, count in ((np.nan, 1), (np.inf, 1), (-np.inf, 1)):
        x = np.ones(10, np.float32)
        x[7] = bad
        on = gn.state_after([x], 1.0, gn.CLIP | gn.SKIP_NONFINITE, steps=4, skipped_steps=1)
        off = gn.state_after([x], 1.0, gn.CLIP, steps=4, skipped_steps=1)
        assert on["nonfinite"] == off["nonfinite"] == count and on["skip"] == 1 and off["skip"] == 0
        assert (on["steps"], on["skipped_steps"], off["skipped_steps"]) == (5, 2, 1)
        assert np.isnan(on["coef"]) if np.isnan(bad) else on["coef"] == 0.0
    assert gn.state_after(one, 1.0, gn.SKIP_NONFINITE, user_guard=-3)["skip"] == 1 and gn.state_after(one, 1.0, 0, user_guard=1)["skip"] == 1


def test_clipped_update_is_torch_mul_then_torch_sgd_bit_for_bit():
    """Five steps, two tensors, momentum and weight decay: torch on the CPU scales the gradient in place (g.mul_(coef), what
    clip_grad_norm_ does) and steps; the restatement gets round(g * coef) -- what sgd_update_kernel<true> forms in registers."""
    g0 = torch.Generator().manual_seed(5)
    shapes, lr, mu, wd = [(37,), (5, 11)], 2e-3, 0.9, 5e-4
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g0) * 0.1) for s in shapes]
    opt = torch.optim.SGD(ps, lr=lr, momentum=mu, weight_decay=wd)
    mine = [(p.detach().numpy().copy().reshape(-1), np.zeros(p.numel(), np.float32), 0) for p in ps]
    seen = set()
    for step, max_norm in enumerate((10.0, 0.05, 0.05, 1e-3, 10.0)):
        grads = [torch.randn(*s, generator=g0) * 0.02 for s in shapes]
        if step == 3:
            grads[0][5] = 1e-41                                            # a subnormal product
        st = gn.state_after([g.numpy() for g in grads], max_norm, gn.CLIP)
        coef = st["coef"]
        seen.add(bool(coef < 1))
        for p, g in zip(ps, grads):
            p.grad = g.clone()
            p.grad.mul_(torch.tensor(coef))
        opt.step()
        for k, (g, (p, m, born)) in enumerate(zip(grads, mine)):
            scaled = (g.numpy().reshape(-1) * np.float32(coef)).astype(np.float32)
            mine[k] = sgd_ref.sgd_update(p, scaled, m, born, lr, mu, wd)
            assert np.array_equal(sgd_ref.bits(mine[k][0]), sgd_ref.bits(ps[k].detach().numpy().reshape(-1))), (step, k)
            assert np.array_equal(sgd_ref.bits(mine[k][1]), sgd_ref.bits(opt.state[ps[k]]["momentum_buffer"].numpy().reshape(-1))), (step, k)
    assert seen == {True, False}


@pytest.fixture(scope="module")
def L():
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def test_workspace_bytes(L):
    f = L.lib.frcnn_grad_norm_workspace_bytes
    assert f(-1) == 0 and f(-2 ** 31) == 0
    assert f(0) == 16 and f(1) == 16 and f(2) == 32 and f(123) == (123 * 12 + 15) // 16 * 16
    assert f(2 ** 31 - 1) >= 12 * (2 ** 31 - 1)


def test_grad_norm_refuses_bad_arguments_before_touching_the_device(L):
    f = L.lib.frcnn_grad_norm
    T, S, W = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)                         # never dereferenced on the host
    need, ws = 64 + 48 * 3 + 8 * 5, int(L.lib.frcnn_grad_norm_workspace_bytes(5))
    for args, text in (((None, need, 3, 5, S, None, W, ws, None), "NULL pointer"), ((T, need, 3, 5, None, None, W, ws, None), "NULL pointer"),
                       ((T, need, 3, 5, S, None, None, ws, None), "NULL pointer"), ((T, need, 0, 5, S, None, W, ws, None), "bad counts"),
                       ((T, need, 65537, 5, S, None, W, ws, None), "bad counts"), ((T, need, 3, -1, S, None, W, ws, None), "bad counts"),
                       ((C.c_void_p(0x1008), need, 3, 5, S, None, W, ws, None), "aligned"), ((T, need, 3, 5, C.c_void_p(0x2004), None, W, ws, None), "aligned"),
                       ((T, need, 3, 5, S, None, C.c_void_p(0x3008), ws, None), "aligned"), ((T, need, 3, 5, S, C.c_void_p(0x4002), W, ws, None), "aligned")):
        assert f(*args) == -1 and text.encode() in L.lib.frcnn_last_error(), args
    assert f(T, need - 1, 3, 5, S, None, W, ws, None) == -3 and b"short table" in L.lib.frcnn_last_error()
    assert f(T, need, 3, 5, S, None, W, ws - 1, None) == -3 and b"short workspace" in L.lib.frcnn_last_error()
    assert f(T, 64 + 48 * 3, 3, 0, S, None, W, 15, None) == -3 and b"short workspace" in L.lib.frcnn_last_error()


def test_scaled_step_refuses_bad_arguments_before_touching_the_device(L):
    f = L.lib.frcnn_sgd_step_scaled
    T, H, B, K, G = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))
    need = 64 + 48 * 3 + 8 * 5
    for args, text in (((T, need, 3, 5, H, 1, B, K, None, None), "NULL pointer"), ((None, need, 3, 5, H, 1, B, K, G, None), "NULL pointer"),
                       ((T, need, 3, 5, None, 1, B, K, G, None), "NULL pointer"), ((T, need, 3, 5, H, 1, None, K, G, None), "NULL pointer"),
                       ((T, need, 0, 5, H, 1, B, K, G, None), "bad counts"), ((T, need, 3, -1, H, 1, B, K, G, None), "bad counts"),
                       ((T, need, 3, 5, H, 0, B, K, G, None), "n_groups"), ((T, need, 3, 5, H, 1, B, K, C.c_void_p(0x5002), None), "aligned"),
                       ((T, need, 3, 5, H, 1, B, C.c_void_p(0x4001), G, None), "aligned")):
        assert f(*args) == -1 and text.encode() in L.lib.frcnn_last_error() and b"sgd_step_scaled" in L.lib.frcnn_last_error(), args
    assert f(T, need - 1, 3, 5, H, 1, B, K, G, None) == -3 and b"short table" in L.lib.frcnn_last_error()


def test_device_sgd_refuses_a_bad_max_grad_norm_or_norm_type(L):
    from faster_rcnn_pytorch_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in (0, 0.0, -1.0, float("nan"), torch.tensor(1.0), "1", True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            optim.DeviceSGD([p], lr=0.1, max_grad_norm=bad)
    for bad in (1, 1.0, float("inf"), 3.0, "inf", torch.tensor(2.0)):
        with pytest.raises(ValueError, match="norm_type"):
            optim.DeviceSGD([p], lr=0.1, max_grad_norm=1.0, norm_type=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # valid options: the device check comes next, as without them
        optim.DeviceSGD([p], lr=0.1, max_grad_norm=1.0, skip_nonfinite=True, norm_type=2)
    assert struct_size(optim.GN_STATE_FORMAT) == optim.GN_STATE_BYTES == 64


def struct_size(fmt):
    import struct
    return struct.calcsize(fmt)
