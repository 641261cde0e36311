"""CPU-only checks of the device-side SGD (csrc/sgd.hip, faster_rcnn_pytorch_amd/optim.py):

  * the numpy restatement of the update rule (tests/sgd_ref.py, error-free fused operations) equals tests/golden/sgd.npz --
    torch.optim.SGD run on the CPU -- bit for bit, NaN by position, on every case and every step;
  * fma32 itself on operands where a binary64 sum narrowed to binary32 rounds twice;
  * the host-side table builder's refusals through the C ABI (no device is touched);
  * DeviceSGD's parameter-group keys against torch.optim.SGD's, and its refusal of CPU tensors (no fallback)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sgd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sgd.npz")


@pytest.fixture(scope="module")
def cases():
    return sgd_ref.load_cases(GOLDEN)


def test_golden_file_holds_every_kind_of_case(cases):
    names = [c.name for c in cases]
    assert names == ["lengths_five_steps", "wd0_inf_parameter", "momentum_zero", "two_groups", "chunk_edges", "three_hundred_tensors", "long_tensor", "sweep_seams"]
    by = dict(zip(names, cases))
    assert by["lengths_five_steps"].lens.tolist() == [1, 3, 4, 5, 63, 64, 65, 255, 256, 257] and by["lengths_five_steps"].steps == 5
    assert by["chunk_edges"].lens.tolist() == [8191, 8192, 8193]
    assert by["sweep_seams"].lens.tolist() == [1023, 1024, 1025, 4095, 4096, 4097, 4100]
    assert len(by["three_hundred_tensors"].lens) == 300 and by["long_tensor"].total > 1000000
    a = by["lengths_five_steps"]
    assert a.hyper[1, 0, 0] != a.hyper[2, 0, 0] and np.isnan(a.g).sum() == 1 and (np.signbit(a.g) & (a.g == 0)).sum() >= 4
    assert np.isinf(by["wd0_inf_parameter"].p0).sum() == 3 and (by["wd0_inf_parameter"].hyper[:, :, 2] == 0).all()
    assert (by["momentum_zero"].hyper[:, :, 1] == 0).all() and not by["momentum_zero"].born.any()
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_restatement_equals_torch_cpu_bit_for_bit(cases):
    for c in cases:
        ps, ms, bs = sgd_ref.run_reference(c)
        for s in range(c.steps):
            assert sgd_ref.sha(ps[s]) == c.sha_p[s], (c.name, s, "parameters")
            assert sgd_ref.sha(ms[s]) == c.sha_m[s], (c.name, s, "momentum")
            assert np.array_equal(bs[s], c.born[s]), (c.name, s, "born")
        if c.p_final is not None:
            assert np.array_equal(sgd_ref.bits(ps[-1]), sgd_ref.bits(c.p_final)) and np.array_equal(sgd_ref.bits(ms[-1]), sgd_ref.bits(c.m_final))
            assert np.array_equal(np.isnan(ps[-1]), np.isnan(c.p_final))


def test_fma32_rounds_once():
    f = np.float32
    # a * b = 1 - 2^-30, c = 2^24 + 2 (an odd significand; binary32 spacing there is 2): the exact sum 2^24 + 3 - 2^-30 lies just below the
    # tie and rounds to 2^24 + 2.  Binary64 (spacing 2^-28) rounds it to the tie 2^24 + 3, which then narrows to even: 2^24 + 4.
    a, b, c = f(1 + 2.0 ** -15), f(1 - 2.0 ** -15), f(2.0 ** 24 + 2)
    assert float(np.float64(a) * np.float64(b)) == 1 - 2.0 ** -30
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == f(2.0 ** 24 + 4)       # rounded twice
    assert sgd_ref.fma32(a, b, c) == f(2.0 ** 24 + 2)                                          # rounded once
    assert sgd_ref.fma32(-a, b, -c) == f(-(2.0 ** 24 + 2))
    assert sgd_ref.fma32(np.array([a, -a]), np.array([b, b]), np.array([c, -c])).tolist() == [2.0 ** 24 + 2, -(2.0 ** 24 + 2)]
    # special values and the subnormal range
    assert np.isnan(sgd_ref.fma32(f(0), f(np.inf), f(1))) and sgd_ref.fma32(f(2), f(np.inf), f(1)) == f(np.inf)
    assert sgd_ref.fma32(f(-2e-3), f(1e-37), f(3e-38)) == f(np.float64(f(-2e-3)) * np.float64(f(1e-37)) + np.float64(f(3e-38)))
    tiny = sgd_ref.fma32(f(2.0 ** -100), f(2.0 ** -49), f(2.0 ** -149))                        # 2^-149 + 2^-149: exact, subnormal
    assert tiny == f(2.0 ** -148)
    assert np.signbit(sgd_ref.fma32(f(-0.0), f(1), f(-0.0))) and not np.signbit(sgd_ref.fma32(f(-0.0), f(1), f(0.0)))


@pytest.fixture(scope="module")
def L():
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def _build(L, params, grads, moms, numel, group, n_groups, table_bytes=None, n=None):
    n = len(numel) if n is None else n
    vp = C.c_void_p * max(len(numel), 1)
    ne = (C.c_int64 * max(len(numel), 1))(*numel)
    need = int(L.lib.frcnn_sgd_table_bytes(n, ne))
    size = need if table_bytes is None else table_bytes
    buf = (C.c_uint8 * max(size, 64))()
    nch = C.c_int32(-1)
    rc = L.lib.frcnn_sgd_table_build_host(n, vp(*params), vp(*grads), vp(*moms), ne, (C.c_int32 * max(len(numel), 1))(*group), n_groups,
                                          buf, size, C.byref(nch))
    return rc, (L.lib.frcnn_last_error() or b"").decode(), nch.value, need, bytes(buf[:size])


def test_table_builder_layout_and_refusals(L):
    P, G, M = 0x10000000, 0x20000000, 0x30000000                        # never dereferenced on the host
    numel = [1, 8192, 8193, 0, 20000]
    ps = [P + 0x100000 * i for i in range(5)]
    gs = [G + 0x100000 * i for i in range(5)]
    ms = [M + 0x100000 * i for i in range(5)]
    rc, msg, nch, need, tab = _build(L, ps, gs, ms, numel, [0, 1, 0, 1, 1], 2)
    assert rc == 0 and nch == 1 + 1 + 2 + 0 + 3 and need == 64 + 48 * 5 + 8 * nch
    rows = np.frombuffer(tab, np.int64, 6 * 5, 64).reshape(5, 6)
    assert rows[:, 0].tolist() == ps and rows[:, 1].tolist() == gs and rows[:, 2].tolist() == ms and rows[:, 3].tolist() == numel
    grp_vec = np.frombuffer(tab, np.int32, 12 * 5, 64).reshape(5, 12)[:, 8:10]
    assert grp_vec[:, 0].tolist() == [0, 1, 0, 1, 1] and grp_vec[:, 1].tolist() == [1] * 5
    cmap = np.frombuffer(tab, np.int32, 2 * nch, 64 + 48 * 5).reshape(nch, 2)
    assert cmap.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [4, 0], [4, 1], [4, 2]]
    rc, _, _, _, tab = _build(L, [ps[0] + 4] + ps[1:], gs, ms, numel, [0] * 5, 1)                  # a view at a storage offset of one float
    assert rc == 0 and np.frombuffer(tab, np.int32, 12 * 5, 64).reshape(5, 12)[:, 9].tolist() == [0, 1, 1, 1, 1]
    assert L.lib.frcnn_sgd_table_bytes(0, (C.c_int64 * 1)(1)) == 0 and L.lib.frcnn_sgd_table_bytes(1, (C.c_int64 * 1)(-1)) == 0
    bad = [
        (dict(numel=[1, -5, 3, 0, 2]), "negative size"),
        (dict(params=[ps[0], 0] + ps[2:]), "NULL pointer in row 1"),
        (dict(grads=gs[:4] + [0]), "NULL pointer in row 4"),
        (dict(moms=[0] + ms[1:]), "NULL pointer in row 0"),
        (dict(moms=[ps[1] + 4 * 100] + ms[1:]), "overlapping parameter and momentum"),
        (dict(moms=ms[:4] + [ps[4] + 4 * 19999]), "overlapping parameter and momentum"),
        (dict(params=ps[:4] + [ps[1]]), "overlapping parameter and momentum"),
        (dict(grads=[gs[0], ps[1] + 4] + gs[2:]), "gradient of row 1 overlaps"),
        # the shared disjointness check (csrc/multi_tensor_dev.h), branch by branch: rows 1 and 2 hold 8192 and 8193 elements
        (dict(moms=[ms[0], ms[2] - 4 * 8191] + ms[2:]), "overlapping parameter and momentum (m of row 1 and m of row 2)"),      # one element shared
        (dict(grads=[gs[0], ps[2] + 4 * 8192] + gs[2:]), "gradient of row 1 overlaps"),          # its first element is the last of p of row 2
        (dict(grads=[gs[0], ps[2] - 4 * 8191] + gs[2:]), "gradient of row 1 overlaps"),          # its last element is the first of p of row 2
        (dict(group=[0, 1, 2, 0, 0]), "names group 2 outside 0 .. 1"),
        (dict(group=[0, -1, 0, 0, 0]), "names group -1"),
        (dict(params=[ps[0] + 2] + ps[1:]), "not 4-byte aligned"),
        (dict(n_groups=0), "n_groups"),
    ]
    for change, text in bad:
        kw = dict(params=ps, grads=gs, moms=ms, numel=numel, group=[0, 1, 0, 1, 1], n_groups=2)
        kw.update(change)
        rc, msg, _, _, _ = _build(L, **kw)
        assert rc == -1 and text in msg, (change, rc, msg)
    for change in (dict(moms=[ms[0], ms[2] - 4 * 8192] + ms[2:]), dict(grads=[gs[0], ps[2] - 4 * 8192] + gs[2:]),
                   dict(grads=[gs[0], ps[2] + 4 * 8193] + gs[2:])):                              # ranges that only touch do not overlap
        kw = dict(params=ps, grads=gs, moms=ms, numel=numel, group=[0, 1, 0, 1, 1], n_groups=2)
        kw.update(change)
        assert _build(L, **kw)[0] == 0, change
    rc, msg, _, need, _ = _build(L, ps, gs, ms, numel, [0, 1, 0, 1, 1], 2, table_bytes=need - 8)
    assert rc == -3 and "short table" in msg
    assert L.lib.frcnn_sgd_table_build_host(5, None, None, None, None, None, 2, None, 0, None) == -1 and b"NULL argument" in L.lib.frcnn_last_error()


def test_step_refuses_bad_arguments_before_touching_the_device(L):
    f = L.lib.frcnn_sgd_step
    T, H, B = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    need = 64 + 48 * 3 + 8 * 5
    for args, text in (((None, need, 3, 5, H, 1, B, None, None), "NULL pointer"), ((T, need, 3, 5, None, 1, B, None, None), "NULL pointer"),
                       ((T, need, 3, 5, H, 1, None, None, None), "NULL pointer"), ((T, need, 0, 5, H, 1, B, None, None), "bad counts"),
                       ((T, need, 3, -1, H, 1, B, None, None), "bad counts"), ((T, need, 3, 5, H, 0, B, None, None), "n_groups"),
                       ((C.c_void_p(0x1008), need, 3, 5, H, 1, B, None, None), "aligned"), ((T, need, 3, 5, H, 1, B, C.c_void_p(0x3002), None), "aligned")):
        assert f(*args) == -1 and text.encode() in L.lib.frcnn_last_error(), args
    assert f(T, need - 1, 3, 5, H, 1, B, None, None) == -3 and b"short table" in L.lib.frcnn_last_error()


def test_device_sgd_group_keys_are_torch_sgd_s_and_cpu_tensors_are_refused(L):
    from faster_rcnn_pytorch_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    ref = torch.optim.SGD([p], lr=2e-3, momentum=0.9, weight_decay=5e-4)
    mine = optim.group_defaults(lr=2e-3, momentum=0.9, weight_decay=5e-4)
    theirs = {k: v for k, v in ref.state_dict()["param_groups"][0].items() if k != "params"}
    assert list(mine) == list(theirs) == list(optim.GROUP_KEYS) and mine == theirs
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.DeviceSGD([p], lr=2e-3, momentum=0.9)
    for kw in (dict(dampening=0.1), dict(nesterov=True, momentum=0.9), dict(maximize=True)):
        with pytest.raises(ValueError, match="not supported"):
            optim.DeviceSGD([p], lr=2e-3, **kw)
