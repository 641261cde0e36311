"""The scalar journal on the GPU (csrc/telemetry.hip: frcnn_journal_append, through telemetry.ScalarJournal): ring, marks, totals and
cursor equal the numpy restatement (tests/journal_ref.py) bit for bit, and smoothed() returns what the reference's SmoothedValue returned
for the golden series (tests/golden/journal.npz) after they went through the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded
import journal_ref as jr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}
KEYS = ("median", "max", "value", "global_avg", "count", "avg")


def _journal(names, capacity):
    from faster_rcnn_pytorch_amd.telemetry import ScalarJournal
    return ScalarJournal(names, capacity, DEV)


def _assert_equal(j, ref, last=None):
    got = j.read(last)
    rows, marks = ref.rows(last)
    assert got["cursor"] == ref.cursor and got["names"] == j.names
    assert np.array_equal(jr.bits(got["rows"]), jr.bits(rows)) and np.array_equal(got["marks"], marks)
    for c, name in enumerate(j.names):
        t = got["totals"][name]
        assert jr.bits(np.array([t["sum"], t["max"], t["min"]])).tolist() == jr.bits(np.array([ref.sum[c], ref.max[c], ref.min[c]])).tolist(), name
        assert (t["count"], t["nonfinite"]) == (int(ref.count[c]), int(ref.nonfinite[c])), name
    return got


def _row(k):
    """Four dtypes in one row; NaN and both infinities on the way; an int64 that binary64 must round."""
    x = np.float32(k) * np.float32(0.37) - np.float32(2)
    row = [x, np.float64(k) / 3 - 1, np.int32(7 - 3 * k), np.int64(2 ** 53 + 1 + 2 * k)]
    if k == 4:
        row[0] = np.float32(np.nan)
    if k == 6:
        row[0], row[1] = np.float32(-np.inf), np.float64(np.inf)
    return row


@pytest.mark.parametrize("appends", [3, 8, 9, 20])
def test_capacity_eight_wraps_with_four_dtypes_marks_and_non_finite_values(appends):
    names = ["f32", "f64", "i32", "i64"]
    j, ref = _journal(names, 8), jr.Journal(4, 8)
    dtypes = (torch.float32, torch.float64, torch.int32, torch.int64)
    src = [torch.zeros(1, dtype=d, device=DEV) for d in dtypes]
    mark = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(appends):
        row = _row(k)
        for s, v in zip(src, row):
            s.copy_(torch.from_numpy(np.array([v])))
        mark.fill_(1000 + k)
        with_mark = k % 3 != 2                                            # every third row without a mark word: 0
        j.append(src, mark if with_mark else None)
        ref.append(row, 1000 + k if with_mark else 0)
    got = _assert_equal(j, ref)
    assert len(got["rows"]) == min(appends, 8)
    _assert_equal(j, ref, last=2), _assert_equal(j, ref, last=0)
    if appends == 20:
        assert got["totals"]["f32"]["nonfinite"] == 2 and got["totals"]["f64"]["nonfinite"] == 1 and got["totals"]["i64"]["count"] == 20
        assert got["rows"][-1, 3] == float(2 ** 53 + 40)                  # 2^53 + 39 rounds to even
    j.reset()
    _assert_equal(j, jr.Journal(4, 8))


@pytest.mark.parametrize("n_cols,capacity", [(1, 1), (64, 3)])
def test_one_and_sixty_four_columns(n_cols, capacity):
    rs = np.random.RandomState(n_cols)
    j, ref = _journal(["c%d" % c for c in range(n_cols)], capacity), jr.Journal(n_cols, capacity)
    dts = [(torch.float32, torch.float64, torch.int32, torch.int64)[c % 4] for c in range(n_cols)]
    block = [torch.zeros(3, dtype=d, device=DEV) for d in dts]             # the source is element 1: values beside it are not read
    for k in range(5):
        vals = [NP_OF[d](rs.randint(-1000, 1000)) if not d.is_floating_point else NP_OF[d](rs.standard_normal()) for d in dts]
        for b, v in zip(block, vals):
            b.copy_(torch.from_numpy(np.array([np.nan if b.is_floating_point() else -1, v, np.nan if b.is_floating_point() else -1]).astype(v.dtype)))
        j.append([b[1:2] for b in block])
        ref.append(vals)
    _assert_equal(j, ref)


@pytest.mark.parametrize("capacity", [20, 64])
def test_smoothed_after_the_golden_series_went_through_the_device(golden, capacity):
    z = golden("journal")
    window, names = int(z["window"]), sorted(z["names"].tolist())
    src = torch.zeros(1, dtype=torch.float32, device=DEV)
    for name in names:                                                    # the series differ in length: one journal each
        j = _journal([name], capacity)
        for v in z[name + "_values"]:
            src.fill_(float(v))
            j.append([src])
        data = j.read()
        assert data["totals"][name]["sum"] == z[name + "_total"] and data["cursor"] == len(z[name + "_values"])      # SmoothedValue.total, bit for bit
        got = j.smoothed(window, data)[name]
        for k in KEYS:
            assert got[k] == z["%s_%s" % (name, k)], (name, k, got[k], z["%s_%s" % (name, k)])
        assert j.smoothed(window)[name] == got


def test_guard_bands_and_a_foreign_state():
    vals = [torch.tensor([1.5], device=DEV), torch.tensor([-7], dtype=torch.int64, device=DEV)]

    def case(g):
        j = _journal(["a", "b"], 4)                                        # the block comes from an arena
        src = [g.place(v) for v in vals]
        for _ in range(6):
            j.append(src)
        return dict(block=j._block, a=src[0], b=src[1])
    a, _ = guarded.run_both(case)
    assert float(a["a"]) == 1.5 and int(a["b"]) == -7
    j = _journal(["a", "b"], 4)
    j._block[8:12].view(torch.int32).fill_(5)                              # the block says capacity 5, the call 4: not ours
    before = j._block.clone()
    j.append(vals)
    torch.cuda.synchronize()
    assert torch.equal(j._block, before)


def test_refusals_through_python_and_the_c_abi():
    from faster_rcnn_pytorch_amd import _lib
    j = _journal(["a", "b"], 4)
    ok = [torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)]
    for bad, exc, text in (([ok[0]], ValueError, "1 values for 2 columns"), ([ok[0], 3.0], TypeError, "b is not a dense tensor"),
                           ([ok[0], torch.zeros(1, dtype=torch.int32)], RuntimeError, "no CPU fallback"),
                           ([ok[0], torch.zeros(2, dtype=torch.int32, device=DEV)], ValueError, "one-element tensors only"),
                           ([ok[0].half(), ok[1]], TypeError, "float32, float64, int32 and int64 only"),
                           ([ok[0], ok[1].bool()], TypeError, "float32, float64, int32 and int64 only")):
        with pytest.raises(exc, match=text):
            j.append(bad)
    with pytest.raises(TypeError, match="mark is torch.int64: int32 only"):
        j.append(ok, mark=torch.zeros(1, dtype=torch.int64, device=DEV))
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="last must be None or an int >= 0"):
            j.read(bad)
    base = j._block.data_ptr()
    src = (C.c_void_p * 2)(base + j._off_ring + 8, ok[1].data_ptr())       # a source inside the ring
    rc = _lib.lib.frcnn_journal_append(2, src, (C.c_int32 * 2)(1, 2), 4, C.c_void_p(base + j._off_ring), C.c_void_p(base + j._off_marks),
                                       C.c_void_p(base + j._off_totals), C.c_void_p(base), None, None)
    assert rc == -1 and b"overlaps" in _lib.lib.frcnn_last_error()
    torch.cuda.synchronize()
    assert j.read()["cursor"] == 0
