"""Host checks of the training telemetry: tests/tensor_stats_ref.py (the restatement of frcnn_tensor_stats) on exact data -- small
integers times a power of two, every sum exact, so each sumsq must EQUAL the integer result -- its state rules, and the refusals of
faster_rcnn_pytorch_amd/telemetry.py and of the C ABI that need no device."""
import ctypes as C
import struct

import numpy as np
import pytest

import grad_norm_ref as gn
import tensor_stats_ref as ts

LENS = [0, 1, 3, 4, 5, 8191, 8192, 8193, 257 * 8192 - 5]


def test_the_restatement_sums_exact_data_exactly():
    rs = np.random.RandomState(31)
    scale = 2.0 ** -9
    for n in LENS:
        ints = [rs.randint(-40, 41, n).astype(np.int64) for _ in range(3)]
        g, p, m = [(v * scale).astype(np.float32) for v in ints]
        r = ts.row_of(g, p, m, born=1)
        for key, v in zip(("g_sumsq", "p_sumsq", "m_sumsq"), ints):
            exact = int((v * v).sum())
            assert exact < 2 ** 53 and r[key] == exact * scale * scale, (n, key)
        assert r["g_absmax"] == np.float32(np.abs(ints[0]).max() * scale if n else 0) and r["p_absmax"] == np.float32(np.abs(ints[1]).max() * scale if n else 0)
        assert (r["g_nonfinite"], r["p_nonfinite"], r["m_read"]) == (0, 0, int(n > 0))
        u = ts.row_of(g, p, np.full(n, np.nan, np.float32), born=0)                   # unborn: the momentum is not looked at
        assert u["m_sumsq"] == 0 and u["m_read"] == 0 and ts.row_bits(u)[:2] == ts.row_bits(r)[:2]


def test_the_per_tensor_tree_is_the_global_tree_on_one_small_tensor_and_differs_in_depth_only():
    rs = np.random.RandomState(32)
    x = (rs.standard_normal(3 * 8192 + 17) * 0.02).astype(np.float32)
    part, _ = gn.chunk_partials(x)
    assert ts.partials_of(x)[0].tobytes() == part.tobytes()                          # the chunk contract is grad_norm's
    # 4 partials: threads 0 .. 3 of wave 0 hold one each in both trees, and the other waves add +0
    assert gn.f64_bits(ts.tensor_sumsq(part)) == gn.f64_bits(gn.finish(part, np.zeros(4, np.int32))[0])
    assert ts.additions_per_tensor(8192) == 8 + 2 + 6 + 3 + 1 + 6 + 3 and ts.additions_per_tensor(257 * 8192) == 8 + 2 + 6 + 3 + 2 + 6 + 3
    assert ts.additions_per_tensor(1) == 1 + 2 + 6 + 3 + 1 + 6 + 3


def test_maxima_and_counts_with_non_finite_values():
    x = np.array([1.0, -3.0, np.nan, 2.0], np.float32)
    assert ts.absmax_of(x) == 3.0 and ts.absmax_of(np.array([np.nan], np.float32)) == 0.0 and ts.absmax_of(np.zeros(0, np.float32)) == 0.0
    y = np.array([1.0, -np.inf, np.nan], np.float32)
    assert ts.absmax_of(y) == np.inf
    r = ts.row_of(y, x, x, born=1)
    assert (r["g_nonfinite"], r["p_nonfinite"]) == (2, 1) and np.isnan(r["g_sumsq"]) and np.isnan(r["m_sumsq"])
    assert ts.row_bits(r)[0] == "nan" and ts.row_bits(ts.row_of(np.array([np.inf], np.float32), x, x, 0))[0] == "+inf"


def test_state_rules_every_three_over_seven_calls():
    st = ts.State(3, 2)
    a = [np.array([3.0, 4.0], np.float32), np.zeros(0, np.float32)]
    seen = []
    for k in range(7):
        g = [a[0] * np.float32(k + 1), a[1]]
        if k == 3:
            g[0] = np.array([np.nan, 1.0], np.float32)
        measured = st.call(g, a, a, [1, 0])
        seen.append((measured, st.words(), st.rows[0]["g_sumsq"] if not np.isnan(st.rows[0]["g_sumsq"]) else None))
    assert [m for m, _, _ in seen] == [True, False, False, True, False, False, True]
    assert seen[2][1] == (3, 3, 0, 1, -1, -1) and seen[2][2] == 25.0
    assert seen[3][1] == (3, 4, 3, 2, 0, -1) and seen[5][1] == (3, 6, 3, 2, 0, -1)
    assert seen[6][1] == (3, 7, 6, 3, -1, -1) and seen[6][2] == 25.0 * 49
    assert st.rows[1] == dict(g_sumsq=0.0, p_sumsq=0.0, m_sumsq=0.0, g_absmax=0.0, p_absmax=0.0, g_nonfinite=0, p_nonfinite=0, m_read=0)
    foreign = ts.State(0, 2)
    assert foreign.call(a, a, a, [1, 0]) is False and foreign.words() == (0, 0, -1, 0, -1, -1) and foreign.rows is None


def test_python_refusals_that_need_no_device():
    import torch
    from faster_rcnn_pytorch_amd import telemetry as tm
    with pytest.raises(TypeError, match="must be a DeviceSGD"):
        tm.TensorStats(torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.1))
    for bad in (0, -1, 2.0, True, torch.tensor(3), 2 ** 31):
        with pytest.raises(ValueError, match="every must be a Python int >= 1"):
            tm._check_every(bad)
    assert tm._check_every(7) == 7
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tm.ScalarJournal(["loss"], 8, "cpu")
    for names in ([], ["a"] * 2, ["c%d" % k for k in range(65)], [1, 2]):
        with pytest.raises(ValueError, match="names must be 1 .. 64 distinct strings"):
            tm.ScalarJournal(names, 8, "cuda:0")
    for cap in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="capacity must be an int >= 1"):
            tm.ScalarJournal(["a"], cap, "cuda:0")
    with pytest.raises(ValueError, match="window must be an int >= 1"):
        tm.ScalarJournal.smoothed(None, window=0)


def test_decode_reads_the_block_by_the_documented_offsets():
    from faster_rcnn_pytorch_amd import telemetry as tm
    block = np.zeros(64 + 2 * 64, np.uint8)
    struct.pack_into("<iiiiii", block, 0, 5, 11, 10, 3, 1, -1)
    struct.pack_into("<dddffiii", block, 64, 9.0, 16.0, 0.0, 3.0, 4.0, 0, 0, 0)
    struct.pack_into("<dddffiii", block, 128, float("nan"), 4.0, 25.0, float("inf"), 2.0, 2, 0, 1)
    out = tm.TensorStats.decode(block, ["conv.weight", "conv.bias"])
    assert (out["every"], out["tick"], out["measured_tick"], out["measures"]) == (5, 11, 10, 3)
    assert out["first_nonfinite_g"] == "conv.bias" and out["first_nonfinite_g_index"] == 1 and out["first_nonfinite_p"] is None
    a, b = out["tensors"]["conv.weight"], out["tensors"]["conv.bias"]
    assert (a["grad_norm"], a["weight_norm"], a["momentum_norm"], a["grad_absmax"], a["weight_absmax"], a["momentum_read"]) == (3.0, 4.0, 0.0, 3.0, 4.0, 0)
    assert np.isnan(b["grad_norm"]) and b["momentum_norm"] == 5.0 and b["grad_absmax"] == np.inf and b["grad_nonfinite"] == 2 and b["momentum_read"] == 1


def test_c_abi_refusals_before_any_launch():
    from faster_rcnn_pytorch_amd import _lib
    L = _lib.lib
    assert L.frcnn_tensor_stats_workspace_bytes(1, 0) == 16 and L.frcnn_tensor_stats_workspace_bytes(3, 5) == 208
    assert L.frcnn_tensor_stats_workspace_bytes(0, 5) == 0 and L.frcnn_tensor_stats_workspace_bytes(65537, 5) == 0 and L.frcnn_tensor_stats_workspace_bytes(1, -1) == 0
    vp = C.c_void_p
    ok = dict(table=vp(0x1000), bytes=64 + 48 + 8, n=1, c=1, born=vp(0x2000), rows=vp(0x3000), state=vp(0x4000), ws=vp(0x5000), wsb=48)

    def stats(**kw):
        a = dict(ok, **kw)
        return L.frcnn_tensor_stats(a["table"], a["bytes"], a["n"], a["c"], a["born"], a["rows"], a["state"], a["ws"], a["wsb"], None)
    for kw, rc, text in ((dict(table=None), -1, b"NULL"), (dict(born=None), -1, b"NULL"), (dict(rows=None), -1, b"NULL"), (dict(state=None), -1, b"NULL"),
                         (dict(ws=None), -1, b"NULL"), (dict(n=0), -1, b"bad counts"), (dict(n=65537), -1, b"bad counts"), (dict(c=-1), -1, b"bad counts"),
                         (dict(rows=vp(0x3008)), -1, b"16-byte aligned"), (dict(state=vp(0x4004)), -1, b"16-byte aligned"), (dict(born=vp(0x2002)), -1, b"4-byte aligned"),
                         (dict(bytes=119), None, b"short table"), (dict(wsb=47), None, b"short workspace"),
                         (dict(state=vp(0x3000 + 32)), -1, b"overlap"), (dict(state=vp(0x3000)), -1, b"overlap"), (dict(ws=vp(0x4000 + 16)), -1, b"overlap")):
        got = stats(**kw)
        assert got != 0 and (rc is None or got == rc) and text in L.frcnn_last_error(), (kw, got, L.frcnn_last_error())
    src, dt = (vp * 2)(0x1000, 0x1008), (C.c_int32 * 2)(0, 1)
    okj = dict(n=2, src=src, dt=dt, cap=8, ring=vp(0x10000), marks=vp(0x20000), totals=vp(0x30000), state=vp(0x40000), mark=None)

    def append(**kw):
        a = dict(okj, **kw)
        return L.frcnn_journal_append(a["n"], a["src"], a["dt"], a["cap"], a["ring"], a["marks"], a["totals"], a["state"], a["mark"], None)
    for kw, text in ((dict(n=0), b"n_cols 0 outside"), (dict(n=65), b"n_cols 65 outside"), (dict(cap=0), b"capacity 0 < 1"), (dict(src=None), b"NULL"),
                     (dict(dt=None), b"NULL"), (dict(ring=None), b"NULL"), (dict(marks=None), b"NULL"), (dict(totals=None), b"NULL"), (dict(state=None), b"NULL"),
                     (dict(ring=vp(0x10004)), b"8-byte aligned"), (dict(marks=vp(0x20002)), b"4-byte aligned"), (dict(state=vp(0x40008)), b"16-byte aligned"),
                     (dict(mark=vp(0x50001)), b"4-byte aligned"), (dict(dt=(C.c_int32 * 2)(0, 4)), b"unknown dtype code 4"),
                     (dict(dt=(C.c_int32 * 2)(-1, 0)), b"unknown dtype code -1"), (dict(src=(vp * 2)(0x1000, None)), b"NULL source"),
                     (dict(src=(vp * 2)(0x1002, 0x1008)), b"not 4-byte aligned"), (dict(src=(vp * 2)(0x1000, 0x1004)), b"not 8-byte aligned"),
                     (dict(src=(vp * 2)(0x10000 + 8 * 15, 0x1008)), b"overlaps"), (dict(src=(vp * 2)(0x1000, 0x30000 + 72)), b"overlaps"),
                     (dict(src=(vp * 2)(0x40000 + 60, 0x1008)), b"overlaps"), (dict(src=(vp * 2)(0x20000 + 28, 0x1008)), b"overlaps"),
                     (dict(mark=vp(0x10000)), b"overlaps")):
        assert append(**kw) == -1 and text in L.frcnn_last_error(), (kw, L.frcnn_last_error())
