"""frcnn_tensor_stats (csrc/telemetry.hip) restated in numpy from the pieces of tests/grad_norm_ref.py: the chunk partials are
grad_norm_ref.chunk_partials (the same contract, the same device code), the per-tensor finish is grad_norm_ref.finish's tree with
T = 256 threads over ONE tensor's partials, and the state rules are the ones include/frcnn_hip.h writes down.

    rows_of(g, p, m, born)      one dict per tensor: g_sumsq, p_sumsq, m_sumsq (float64), g_absmax, p_absmax (float32), g_nonfinite,
                                p_nonfinite, m_read
    State(every)                call(g, p, m, born) -> advances tick; on a measuring tick replaces .rows and the first_nonfinite words"""
import numpy as np

import grad_norm_ref as gn

FINISH_THREADS = 256
INT32_MAX = 2 ** 31 - 1


def absmax_of(x):
    """The `>` comparison from +0: a NaN never wins, an inf does."""
    x = np.asarray(x, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        a = a[~np.isnan(a)]
    return np.float32(a.max()) if a.size else np.float32(0)


def partials_of(x):
    """(sums [k] float64, max [k] float32, counts [k] int32) of one tensor's chunks."""
    x = np.asarray(x, np.float32).reshape(-1)
    part, bad = gn.chunk_partials(x)
    mx = np.array([absmax_of(x[c * gn.CHUNK:(c + 1) * gn.CHUNK]) for c in range(len(part))], np.float32)
    return part, mx, bad


def tensor_sumsq(partials):
    """One tensor's finish: 256 threads, thread t adds partials t, t + 256, ...; butterfly inside each of the 4 waves; ((w0 + w1) + w2) + w3."""
    return gn.finish(partials, np.zeros(len(partials), np.int32), T=FINISH_THREADS)[0]


def row_of(g, p, m, born):
    gp, gm, gb = partials_of(g)
    pp, pm, pb = partials_of(p)
    read = bool(born) and np.asarray(g).size > 0
    mp = partials_of(m)[0] if read else np.zeros(len(gp), np.float64)
    return dict(g_sumsq=tensor_sumsq(gp), p_sumsq=tensor_sumsq(pp), m_sumsq=tensor_sumsq(mp) if read else np.float64(0.0),
                g_absmax=np.float32(gm.max()) if len(gm) else np.float32(0), p_absmax=np.float32(pm.max()) if len(pm) else np.float32(0),
                g_nonfinite=min(int(gb.astype(np.int64).sum()), INT32_MAX), p_nonfinite=min(int(pb.astype(np.int64).sum()), INT32_MAX),
                m_read=int(read))


def rows_of(gs, ps, ms, born):
    return [row_of(g, p, m, b) for g, p, m, b in zip(gs, ps, ms, born)]


def first_nonfinite(rows, key):
    return next((t for t, r in enumerate(rows) if r[key] != 0), -1)


def additions_per_tensor(numel):
    """The number of binary64 additions between a square and a tensor's sumsq on the longest path: inside a chunk as
    grad_norm_ref.additions_on_the_longest_path counts them, then ceil(k / 256) partials per finish thread, 6 (butterfly), 3 (waves)."""
    n = int(numel)
    in_chunk = (min(gn.CHUNK, n) + 4 * gn.THREADS - 1) // (4 * gn.THREADS) + 2 + 6 + 3
    return in_chunk + (gn.n_chunks_of(n) + FINISH_THREADS - 1) // FINISH_THREADS + 6 + 3


class State(object):
    """The 64-byte state block and the rows across calls."""

    def __init__(self, every, n_tensors):
        self.every, self.tick, self.measured_tick, self.measures = every, 0, -1, 0
        self.first_nonfinite_g = self.first_nonfinite_p = -1
        self.rows = None                                                  # whatever the caller put there before the first measuring call
        self.n = n_tensors

    def ours(self):
        return self.every >= 1 and self.tick >= 0

    def call(self, gs, ps, ms, born):
        """Returns True when the call measured."""
        if not self.ours():
            return False
        measured = self.tick % self.every == 0
        if measured:
            self.rows = rows_of(gs, ps, ms, born)
            self.measured_tick, self.measures = self.tick, self.measures + 1
            self.first_nonfinite_g = first_nonfinite(self.rows, "g_nonfinite")
            self.first_nonfinite_p = first_nonfinite(self.rows, "p_nonfinite")
        self.tick = (self.tick + 1) & INT32_MAX
        return measured

    def words(self):
        return (self.every, self.tick, self.measured_tick, self.measures, self.first_nonfinite_g, self.first_nonfinite_p)


def row_bits(r):
    """A row as comparable values: finite sums by bit pattern, non-finite sums by class, the rest exactly."""
    def f64(v):
        v = np.float64(v)
        return "nan" if np.isnan(v) else ("+inf" if v > 0 else "-inf") if np.isinf(v) else int(np.array(v).view(np.uint64))
    return (f64(r["g_sumsq"]), f64(r["p_sumsq"]), f64(r["m_sumsq"]), int(np.array(np.float32(r["g_absmax"])).view(np.uint32)),
            int(np.array(np.float32(r["p_absmax"])).view(np.uint32)), int(r["g_nonfinite"]), int(r["p_nonfinite"]), int(r["m_read"]))
