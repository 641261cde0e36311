"""CPU-only checks of the device-side weight average (csrc/ema.hip, optim.WeightEMA):

  * the numpy restatement (tests/ema_ref.py) equals tests/golden/ema.npz -- torch._foreach_lerp_ and AveragedModel on the CPU -- bit for
    bit, NaN by position, on every trajectory and every update, and both branches of the rule are taken;
  * the host-side table builder's layout and refusals through the C ABI (no device is touched), and its map against the SGD table's;
  * the new symbols are declared, exported and bound; WeightEMA's refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ema_ref
import sgd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("frcnn_ema_table_bytes", "frcnn_ema_table_build_host", "frcnn_ema_update", "frcnn_ema_swap", "frcnn_sgd_step_ema")


@pytest.fixture(scope="module")
def z():
    return ema_ref.load()


@pytest.fixture(scope="module")
def L():
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def _same(a, b):
    return np.array_equal(sgd_ref.bits(a), sgd_ref.bits(b)) and np.array_equal(np.isnan(a), np.isnan(b))


def test_golden_file_is_small_and_holds_both_branches_and_special_values(z):
    assert os.path.getsize(ema_ref.GOLDEN) < 256 * 1024
    tr = ema_ref.trajectories(z)
    assert [t[0] for t in tr] == ["warmup_0p9998", "plain_0p9998", "plain_0p3"]
    name, decay, warmup, p, e0, e, w = tr[0]
    assert warmup and p.shape[0] == 12 and (w[:9] >= 0.5).all() and (w[9:] < 0.5).all()          # updates 0-8 large, 9-11 small
    assert (tr[1][6] < 0.5).all() and (tr[2][6] >= 0.5).all()
    both = np.concatenate([e0, p.reshape(-1)])
    assert np.isinf(both).any() and np.isnan(both).any() and (np.signbit(both) & (both == 0)).any()
    assert ((both != 0) & (np.abs(both) < np.finfo(np.float32).tiny)).any()
    assert z["mlp_g"].shape == z["mlp_p"].shape == z["mlp_e"].shape == (12, z["mlp_p0"].size)


def test_schedule_and_restatement_equal_torch_cpu_bit_for_bit(z):
    for name, decay, warmup, p, e0, e, w in ema_ref.trajectories(z):
        st = ema_ref.State(decay, warmup)
        cur = [e0.copy()]
        for k in range(p.shape[0]):
            assert st.w.view(np.uint32) == w[k].view(np.uint32), (name, k)
            cur = st.update([p[k]], cur)
            assert _same(cur[0], e[k]), (name, k)
        assert st.n == p.shape[0] and st.skipped == st.refused == 0
    assert ema_ref.weight(0.9998, True, 0) == np.float32(0.9) and ema_ref.weight(0.9998, True, 8) == np.float32(0.5)
    assert ema_ref.weight(0.9998, True, 10 ** 6) == ema_ref.weight(0.9998, False, 0) == np.float32(1.0 - 0.9998)


def test_restatement_equals_averaged_model_over_an_sgd_run(z):
    lr0, mu, wd = z["mlp_hyper"]
    sizes = [int(np.prod([d for d in s if d])) for s in z["mlp_shapes"]]
    off = np.concatenate([[0], np.cumsum(sizes)])
    p, e = z["mlp_p0"].copy(), z["mlp_p0"].copy()
    m, born = np.zeros_like(p), [0] * len(sizes)
    st = ema_ref.State(float(z["mlp_decay"]), False)
    for k in range(12):
        for t in range(len(sizes)):
            sl = slice(off[t], off[t + 1])
            p[sl], m[sl], born[t] = sgd_ref.sgd_update(p[sl], z["mlp_g"][k, sl], m[sl], born[t], z["mlp_lr"][k], mu, wd)
        e = st.update([p], [e])[0]
        assert _same(p, z["mlp_p"][k]) and _same(e, z["mlp_e"][k]), k
    assert z["mlp_lr"][0] == lr0 and z["mlp_lr"][4] == pytest.approx(lr0 * 0.1) and z["mlp_lr"][8] == pytest.approx(lr0 * 0.01)


def test_skipped_and_refused_updates_of_the_restatement_change_nothing():
    st = ema_ref.State(0.9, True)
    p, e = [np.float32([1, 2, 3])], [np.float32([0, 0, 0])]
    e1 = st.update(p, e)
    e2 = st.update(p, e1, skip=1)
    st.swap()
    e3 = st.update(p, e2)
    st.swap()
    assert _same(e1[0], e2[0]) and _same(e2[0], e3[0]) and not _same(e[0], e1[0])
    assert st.stats() == dict(decay=0.9, num_updates=1, w=float(np.float32(1 - 2 / 11)), warmup=True, swapped=0, skipped=1, refused=1)


def _build(L, params, shadows, numel, table_bytes=None, n=None):
    n = len(numel) if n is None else n
    k = max(len(numel), 1)
    ne = (C.c_int64 * k)(*numel)
    need = int(L.lib.frcnn_ema_table_bytes(n, ne))
    size = need if table_bytes is None else table_bytes
    buf = (C.c_uint8 * max(size, 64))()
    nch = C.c_int32(-1)
    rc = L.lib.frcnn_ema_table_build_host(n, (C.c_void_p * k)(*params), (C.c_void_p * k)(*shadows), ne, buf, size, C.byref(nch))
    return rc, (L.lib.frcnn_last_error() or b"").decode(), nch.value, need, bytes(buf[:size])


def test_table_builder_layout_refusals_and_the_sgd_map(L):
    P, E, G, M = 0x10000000, 0x20000000, 0x30000000, 0x40000000            # never dereferenced on the host
    numel = [1, 8192, 8193, 0, 20000]
    ps, es = [P + 0x100000 * i for i in range(5)], [E + 0x100000 * i for i in range(5)]
    rc, msg, nch, need, tab = _build(L, ps, es, numel)
    assert rc == 0 and nch == 7 and need == 64 + 32 * 5 + 8 * nch
    rows = np.frombuffer(tab, np.int64, 4 * 5, 64).reshape(5, 4)
    assert rows[:, 0].tolist() == ps and rows[:, 1].tolist() == es and rows[:, 2].tolist() == numel
    vec = lambda t: np.frombuffer(t, np.int32, 8 * 5, 64).reshape(5, 8)[:, 6].tolist()   # noqa: E731
    assert vec(tab) == [1] * 5
    hd = np.frombuffer(tab, np.int32, 4, 0)
    assert hd[0] == 0x31414d45 and hd[1:].tolist() == [5, 7, 8192]
    cmap = np.frombuffer(tab, np.int32, 2 * nch, 64 + 32 * 5).reshape(nch, 2)
    # entry for entry the SGD table's map for the same sizes
    vp5, ne = C.c_void_p * 5, (C.c_int64 * 5)(*numel)
    sbytes = int(L.lib.frcnn_sgd_table_bytes(5, ne))
    sbuf, snch = (C.c_uint8 * sbytes)(), C.c_int32(-1)
    assert L.lib.frcnn_sgd_table_build_host(5, vp5(*ps), vp5(*[G + 0x100000 * i for i in range(5)]), vp5(*[M + 0x100000 * i for i in range(5)]), ne,
                                            (C.c_int32 * 5)(0, 0, 0, 0, 0), 1, sbuf, sbytes, C.byref(snch)) == 0
    smap = np.frombuffer(bytes(sbuf), np.int32, 2 * snch.value, 64 + 48 * 5).reshape(snch.value, 2)
    assert snch.value == nch and np.array_equal(cmap, smap) and cmap.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [4, 0], [4, 1], [4, 2]]
    # vec = 1 only when BOTH pointers are 16-byte aligned: a shadow at an odd offset under an aligned parameter, and the other way round
    assert vec(_build(L, ps, [es[0] + 4] + es[1:], numel)[4]) == [0, 1, 1, 1, 1]
    assert vec(_build(L, ps[:2] + [ps[2] + 8] + ps[3:], es, numel)[4]) == [1, 1, 0, 1, 1]
    assert L.lib.frcnn_ema_table_bytes(0, (C.c_int64 * 1)(1)) == 0 and L.lib.frcnn_ema_table_bytes(1, (C.c_int64 * 1)(-1)) == 0
    assert L.lib.frcnn_ema_table_bytes(1, (C.c_int64 * 1)((1 << 40) + 1)) == 0 and L.lib.frcnn_ema_table_bytes(1, None) == 0
    bad = [
        (dict(numel=[1, -5, 3, 0, 2]), "negative size"),
        (dict(numel=[1, (1 << 40) + 1, 3, 0, 2]), "too large"),
        (dict(params=[ps[0], 0] + ps[2:]), "NULL pointer in row 1"),
        (dict(shadows=es[:4] + [0]), "NULL pointer in row 4"),
        (dict(params=[ps[0] + 2] + ps[1:]), "not 4-byte aligned"),
        (dict(shadows=es[:2] + [es[2] + 1] + es[3:]), "not 4-byte aligned"),
        (dict(shadows=[ps[1] + 4 * 100] + es[1:]), "overlapping parameter and shadow"),          # e of row 0 inside p of row 1
        (dict(shadows=es[:4] + [ps[4] + 4 * 19999]), "overlapping parameter and shadow"),        # e of row 4 on the last element of its own p
        (dict(params=ps[:4] + [ps[1]]), "overlapping parameter and shadow"),                     # two p
        (dict(shadows=es[:4] + [es[2] + 4 * 8192]), "overlapping parameter and shadow"),         # two e, one element shared
        (dict(shadows=[es[0], ps[2] - 4 * 8191] + es[2:]), "overlapping parameter and shadow (e of row 1 and p of row 2)"),     # the last of e, the first of p
    ]
    for change, text in bad:
        kw = dict(params=ps, shadows=es, numel=numel)
        kw.update(change)
        rc, msg, _, _, _ = _build(L, **kw)
        assert rc == -1 and text in msg, (change, rc, msg)
    assert _build(L, ps, es[:4] + [es[2] + 4 * 8193], numel)[0] == 0       # touching ranges are no overlap
    assert _build(L, ps, [es[0], ps[2] - 4 * 8192] + es[2:], numel)[0] == 0  # nor an e that ends where a p begins
    rc, msg, _, need, _ = _build(L, ps, es, numel, table_bytes=need - 8)
    assert rc == -3 and "short table" in msg
    assert L.lib.frcnn_ema_table_build_host(5, None, None, None, None, 0, None) == -1 and b"NULL argument" in L.lib.frcnn_last_error()
    assert _build(L, ps, es, numel, n=0)[0] == -1


def test_launches_refuse_bad_arguments_before_touching_the_device(L):
    T, S, H, B, ET = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000), C.c_void_p(0x4000), C.c_void_p(0x5000)
    need, sneed = 64 + 32 * 3 + 8 * 5, 64 + 48 * 3 + 8 * 5
    up, sw, fu = L.lib.frcnn_ema_update, L.lib.frcnn_ema_swap, L.lib.frcnn_sgd_step_ema
    for args, text in (((None, need, 3, 5, S, None, None), "NULL pointer"), ((T, need, 3, 5, None, None, None), "NULL pointer"),
                       ((T, need, 0, 5, S, None, None), "bad counts"), ((T, need, 3, -1, S, None, None), "bad counts"),
                       ((C.c_void_p(0x1008), need, 3, 5, S, None, None), "aligned"), ((T, need, 3, 5, C.c_void_p(0x2004), None, None), "aligned"),
                       ((T, need, 3, 5, S, C.c_void_p(0x3002), None), "aligned")):
        assert up(*args) == -1 and text.encode() in L.lib.frcnn_last_error(), args
    assert up(T, need - 1, 3, 5, S, None, None) == -3 and b"short table" in L.lib.frcnn_last_error()
    assert sw(None, need, 3, 5, S, None) == -1 and sw(T, need, 3, 5, None, None) == -1 and sw(T, need - 1, 3, 5, S, None) == -3
    ok = (T, sneed, 3, 5, H, 1, B, None, None, ET, need, S, None)
    for i, v, rc, text in ((9, None, -1, "NULL pointer"), (11, None, -1, "NULL pointer"), (0, None, -1, "NULL pointer"), (2, 0, -1, "bad counts"),
                           (9, C.c_void_p(0x5008), -1, "aligned"), (11, C.c_void_p(0x2008), -1, "aligned"), (10, need - 1, -3, "short EMA table"),
                           (1, sneed - 1, -3, "short table"), (5, 0, -1, "n_groups")):
        args = list(ok)
        args[i] = v
        assert fu(*args) == rc and text.encode() in L.lib.frcnn_last_error(), (i, v)


def test_new_symbols_are_declared_exported_and_bound_and_the_abi_version_stays(L):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", txt))
    exported = set(re.findall(r" T (frcnn_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()))
    for s in SYMBOLS:
        assert s in declared and s in exported and s in L.SIGNATURES and hasattr(L.lib, s), s
    assert "frcnn_ema_state" in txt and L.lib.frcnn_abi_version() == L.ABI_VERSION == 7 and L.lib.frcnn_layout_check() == 0
    assert "ema.hip" in open(os.path.join(ROOT, "faster_rcnn_pytorch_amd", "csrc", "Makefile")).read()


def test_weight_ema_refusals_that_need_no_device(L):
    import struct

    from faster_rcnn_pytorch_amd import optim
    assert struct.calcsize(optim.EMA_STATE_FORMAT) == optim.EMA_STATE_BYTES == 64
    for n in (0, 1, 8, 9, 1000):
        for warm in (True, False):
            assert np.float32(optim.ema_weight(0.9998, warm, n)) == ema_ref.weight(0.9998, warm, n)
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.WeightEMA([p])
    for bad in (1.0, -0.1, float("nan"), True, "0.9", torch.tensor(0.5)):
        with pytest.raises(ValueError, match="invalid decay"):
            optim.WeightEMA([p], decay=bad)
    with pytest.raises(ValueError, match="no trainable parameter"):
        optim.WeightEMA([torch.zeros(3)])
    with pytest.raises(ValueError, match="no trainable parameter"):
        optim.WeightEMA([{"params": [torch.nn.Parameter(torch.zeros(3), requires_grad=False)]}])
    with pytest.raises(TypeError, match="not a dense strided tensor"):
        optim.WeightEMA([torch.sparse_coo_tensor(torch.zeros(1, 1, dtype=torch.int64), torch.ones(1), (3,)).requires_grad_()])
