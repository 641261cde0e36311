"""Host checks of the scalar journal: tests/journal_ref.py (the restatement of frcnn_journal_append) plus the expressions of
telemetry.smoothed_from against what the reference's own SmoothedValue returned (tests/golden/journal.npz, written by
tests/golden/make_golden_journal.py).  Everything is compared with ==: the values are fp32-representable, the total is a sequential
binary64 sum in append order on both sides."""
import numpy as np
import pytest

import journal_ref as jr

SERIES = ["one", "odd19", "even20", "negative21", "ties45"]
KEYS = ("median", "max", "value", "global_avg", "count", "avg")


def _data(j, names, last=None):
    rows, marks = j.rows(last)
    return dict(cursor=j.cursor, names=list(names), rows=rows, marks=marks,
                totals={n: dict(sum=float(j.sum[c]), count=int(j.count[c]), max=float(j.max[c]), min=float(j.min[c]), nonfinite=int(j.nonfinite[c]))
                        for c, n in enumerate(names)})


@pytest.mark.parametrize("capacity", [20, 64])
@pytest.mark.parametrize("name", SERIES)
def test_smoothed_equals_the_references_smoothed_value(golden, name, capacity):
    from faster_rcnn_pytorch_amd.telemetry import smoothed_from
    z = golden("journal")
    window = int(z["window"])
    values = z[name + "_values"]
    assert values.dtype == np.float32
    j = jr.Journal(1, capacity)
    for k, v in enumerate(values):
        j.append([v], mark=k)
    assert j.sum[0] == z[name + "_total"] and j.count[0] == z[name + "_count"]         # SmoothedValue.total, bit for bit
    got = smoothed_from(_data(j, [name]), window)[name]
    for k in KEYS:
        assert got[k] == z["%s_%s" % (name, k)], (name, k, got[k], z["%s_%s" % (name, k)])
    rows, marks = j.rows()
    assert marks.tolist() == list(range(len(values)))[-capacity:] and np.array_equal(rows[:, 0], values.astype(np.float64)[-capacity:])


def test_the_golden_file_holds_every_kind():
    z = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "journal.npz"))
    assert sorted(len(z[n + "_values"]) for n in SERIES) == [1, 19, 20, 21, 45] and sorted(z["names"].tolist()) == sorted(SERIES)
    assert (z["negative21_values"] < 0).any()
    w = np.sort(z["ties45_values"][-20:])
    assert w[9] == w[10] == z["ties45_median"] and (w == w[9]).sum() >= 3
    w = np.sort(z["even20_values"])
    assert w[9] < w[10] and z["even20_median"] == w[9]                                   # torch.median: the lower middle


def test_ring_wrap_marks_dtypes_and_non_finite_values():
    from faster_rcnn_pytorch_amd.telemetry import smoothed_from
    j = jr.Journal(4, 8)
    for k in range(20):
        x = np.float32(k) * np.float32(0.1)
        row = [x, np.float64(k) / 3, np.int32(-k), np.int64(2 ** 53 + k)]
        if k == 5:
            row[0] = np.float32(np.nan)
        if k == 17:
            row[0], row[1] = np.float32(np.inf), np.float64(-np.inf)
        j.append(row, mark=100 + k)
    rows, marks = j.rows()
    assert j.cursor == 20 and marks.tolist() == list(range(112, 120)) and rows.shape == (8, 4)
    assert np.isinf(rows[5, 0]) and rows[5, 1] == -np.inf and rows[7, 2] == -19.0
    assert rows[1, 3] == float(2 ** 53 + 13) == float(2 ** 53 + 12)                      # int64 -> binary64: round to nearest even
    assert j.nonfinite.tolist() == [2, 1, 0, 0] and j.count.tolist() == [18, 19, 20, 20]
    assert j.max[0] == np.float64(np.float32(19) * np.float32(0.1)) and j.min[2] == -19.0 and j.max[2] == 0.0
    exact = sum(-k for k in range(20))
    assert j.sum[2] == exact
    seq = np.float64(0)
    for k in range(20):
        if k not in (5, 17):
            seq = seq + np.float64(np.float32(k) * np.float32(0.1))
    assert j.sum[0] == seq
    assert len(j.rows(last=3)[0]) == 3 and j.rows(last=3)[1].tolist() == [117, 118, 119] and len(j.rows(last=50)[0]) == 8
    s = smoothed_from(_data(j, ["a", "b", "c", "d"]), 5)
    assert s["c"]["value"] == -19.0 and s["c"]["max"] == -15.0 and s["c"]["median"] == -17.0 and s["c"]["global_avg"] == exact / 20
    short = jr.Journal(1, 8)
    assert smoothed_from(_data(short, ["a"]), 5) == {}                                   # nothing appended: the column is left out
    for k in range(3):
        short.append([np.float32(k)])
    assert short.rows()[1].tolist() == [0, 0, 0] and smoothed_from(_data(short, ["a"]), 5)["a"]["count"] == 3
