"""frcnn_journal_append (csrc/telemetry.hip) restated in numpy: the ring, the marks and the per-column totals of include/frcnn_hip.h.
Every value is widened to binary64 (fp32, int32: exact; int64: round to nearest even, numpy's conversion); a finite value enters sum (one
binary64 addition per append, append order), count, max and min; any other is counted in nonfinite and only lands in the ring."""
import numpy as np


class Journal(object):
    def __init__(self, n_cols, capacity):
        self.n, self.capacity, self.cursor = n_cols, capacity, 0
        self.ring = np.zeros((capacity, n_cols), np.float64)
        self.marks = np.zeros(capacity, np.int32)
        self.sum = np.zeros(n_cols, np.float64)
        self.count = np.zeros(n_cols, np.int64)
        self.max = np.full(n_cols, -np.inf, np.float64)
        self.min = np.full(n_cols, np.inf, np.float64)
        self.nonfinite = np.zeros(n_cols, np.int64)

    def append(self, values, mark=0):
        """values: n numpy scalars of float32 / float64 / int32 / int64."""
        assert len(values) == self.n
        slot = self.cursor % self.capacity
        for c, x in enumerate(values):
            v = np.float64(x)
            self.ring[slot, c] = v
            if np.isfinite(v):
                self.sum[c] = self.sum[c] + v
                self.count[c] += 1
                if v > self.max[c]:
                    self.max[c] = v
                if v < self.min[c]:
                    self.min[c] = v
            else:
                self.nonfinite[c] += 1
        self.marks[slot] = np.int32(mark)
        self.cursor += 1

    def rows(self, last=None):
        """(rows, marks) in append order, oldest first."""
        have = min(self.cursor, self.capacity) if last is None else min(self.cursor, self.capacity, last)
        order = [(self.cursor - have + k) % self.capacity for k in range(have)]
        return self.ring[order].copy(), self.marks[order].copy()


def bits(a):
    """float64 array -> comparable uint64 patterns, every NaN as one."""
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = 0x7FF8000000000000
    return b
