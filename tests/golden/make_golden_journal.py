"""Writes tests/golden/journal.npz: series of fp32-representable values pushed through the REFERENCE's own SmoothedValue
(util/misc.py:27-86, window_size 20), with what its properties return after the last update.

    FRCNN_REFERENCE=<checkout of the reference> python tests/golden/make_golden_journal.py

util/misc.py imports torchvision (for a version check) and packaging at module level; neither is touched by SmoothedValue.  This script
registers a stub `torchvision` with a recent __version__, and a stub `packaging.version` if packaging is absent, then loads the file by
path.  update() is fed Python floats that are widened fp32 values -- what train.py's loss.item() hands it.

Per series s: s_values float32 [n]; s_median, s_avg, s_global_avg, s_max, s_value, s_total float64; s_count int64.  Lengths 1, 19, 20, 21
and 45 at window 20; one series has ties at the median, one has negative values, and the windows of 20 are even-length, where
torch.median takes the lower of the two middle values.  The script asserts that each of those kinds occurs."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WINDOW = 20


def load_smoothed_value():
    ref = os.environ.get("FRCNN_REFERENCE")
    if not ref:
        raise SystemExit("set FRCNN_REFERENCE to a checkout of the reference")
    tv = types.ModuleType("torchvision")
    tv.__version__ = "0.15.0"
    sys.modules.setdefault("torchvision", tv)
    try:
        import packaging.version  # noqa: F401
    except ImportError:
        pk, pv = types.ModuleType("packaging"), types.ModuleType("packaging.version")
        pv.parse = lambda s: tuple(int(x) for x in s.split(".")[:2])
        pk.version = pv
        sys.modules.update({"packaging": pk, "packaging.version": pv})
    spec = importlib.util.spec_from_file_location("ref_util_misc", os.path.join(ref, "util", "misc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SmoothedValue


def make_series():
    rs = np.random.RandomState(20)
    s = {}
    s["one"] = np.array([0.6931472], np.float32)
    s["odd19"] = (rs.rand(19) * 3 + 0.01).astype(np.float32)
    s["even20"] = (rs.rand(20) * 3 + 0.01).astype(np.float32)
    s["negative21"] = (rs.randn(21) * 2).astype(np.float32)
    ties = (rs.rand(45) * 2 + 0.5).astype(np.float32)
    ties[-20:][[1, 4, 7, 9, 12, 15, 18]] = np.float32(1.5)                # seven equal values across the middle of the last window
    ties[-20:][[0, 2, 3, 5, 6, 8, 10]] = rs.rand(7).astype(np.float32) * 0.9 + 0.5     # seven below
    ties[-20:][[11, 13, 14, 16, 17, 19]] = rs.rand(6).astype(np.float32) + 1.6         # six above
    s["ties45"] = ties
    return s


def main():
    SmoothedValue = load_smoothed_value()
    out, kinds = {}, set()
    for name, values in make_series().items():
        sv = SmoothedValue(window_size=WINDOW)
        for v in values:
            sv.update(float(v))                                           # loss.item(): the widened fp32
        out[name + "_values"] = values
        for k in ("median", "avg", "global_avg", "max", "value"):
            out["%s_%s" % (name, k)] = np.float64(getattr(sv, k))
        out[name + "_total"], out[name + "_count"] = np.float64(sv.total), np.int64(sv.count)
        w = np.sort(values[-WINDOW:].astype(np.float64))
        if len(w) % 2 == 0:
            assert sv.median == w[len(w) // 2 - 1] and (w[len(w) // 2] != w[len(w) // 2 - 1] or name == "ties45"), name
            kinds.add("even window: the lower middle")
            if w[len(w) // 2] == w[len(w) // 2 - 1] and (w == sv.median).sum() >= 3:
                kinds.add("ties at the median")
        if (values < 0).any():
            kinds.add("negative values")
        if len(values) > WINDOW:
            kinds.add("longer than the window")
    assert kinds == {"even window: the lower middle", "ties at the median", "negative values", "longer than the window"}, kinds
    assert sorted(len(v) for v in make_series().values()) == [1, 19, 20, 21, 45]
    np.savez(os.path.join(HERE, "journal.npz"), window=np.int64(WINDOW), names=np.array(sorted(make_series())), **out)
    print("wrote journal.npz:", ", ".join(sorted(kinds)))


if __name__ == "__main__":
    main()
