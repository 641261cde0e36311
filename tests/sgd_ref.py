"""The update rule of csrc/sgd.hip restated in numpy, and the reader of tests/golden/sgd.npz (written by tests/golden/make_golden_sgd.py
from torch.optim.SGD on the CPU).

    d  = fma(wd, p, g) if wd != 0 else g
    m' = d on a tensor's first update or with mu == 0, else round(mu * m) + d
    p' = fma(-lr, m', p)

The fused operations round ONCE.  Python 3.10 has no math.fma and a float64 sum narrowed to float32 rounds twice, so fma32 is error-free:
the product of two binary32 values is exact in binary64 (48 significant bits, exponents far inside the range); TwoSum gives the binary64
sum s and its exact error e; where e != 0 the sum is replaced by its round-to-odd value (of s and its neighbour on e's side, the one whose
last significand bit is set), and a round-to-odd binary64 narrows to binary32 -- normal or subnormal -- as the exact value would, because
binary64 carries more than two extra bits (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums", 2008)."""
import hashlib

import numpy as np

F32 = np.float32
CANON_NAN = np.uint32(0x7FC00000)


def fma32(a, b, c):
    """round_binary32(a * b + c), one rounding; a, b, c binary32 (arrays or scalars)."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        prod = a.astype(np.float64) * b.astype(np.float64)                # exact
        cc = np.broadcast_to(c.astype(np.float64), prod.shape)
        s = prod + cc
        bb = s - prod                                                     # TwoSum (Knuth): s + e == prod + cc exactly
        e = (prod - (s - bb)) + (cc - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0)
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix & even, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def sgd_update(p, g, m, born, lr, mu, wd):
    """One tensor, one step.  lr, mu, wd: Python floats as given to the optimizer.  Returns (p', m', born'); m is returned untouched
    when no momentum is kept."""
    lr32, mu32, wd32 = F32(lr), F32(mu), F32(wd)
    with np.errstate(all="ignore"):
        d = fma32(wd32, p, g) if wd32 != 0 else g.copy()
        if mu32 != 0:
            m_new = d.copy() if not born else (mu32 * m).astype(np.float32) + d
            m_out, born = m_new, 1
        else:
            m_new, m_out = d, m
        return fma32(-lr32, m_new, p), m_out, born


def bits(a):
    """The bit patterns with every NaN replaced by one pattern: equality of these is equality bit for bit, NaN by position."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = CANON_NAN
    return u


def sha(a):
    return hashlib.sha256(bits(a).tobytes()).hexdigest()


def seeded_inputs(seed, total, steps):
    """Parameters [total] and gradients [steps, total] of a case that is kept as a seed (numpy's frozen legacy generator)."""
    rs = np.random.RandomState(seed)
    p0 = (rs.standard_normal(total) * 0.1).astype(np.float32)
    g = (rs.standard_normal((steps, total)) * 0.02).astype(np.float32)
    return p0, g


class Case(object):
    """name; lens [T]; group [T]; hyper [S, G, 3] float64 (lr, momentum, weight_decay of every step); p0 [N]; g [S, N];
    expected: sha_p / sha_m [S] (momentum of an unborn tensor hashed as zeros), born [S, T], p_final / m_final [N] or None."""

    def __init__(self, z, i):
        k = "c%d_" % i
        self.name = str(z[k + "name"])
        self.lens = z[k + "lens"].astype(np.int64)
        self.group = z[k + "group"].astype(np.int32)
        self.hyper = z[k + "hyper"].astype(np.float64)
        self.steps = self.hyper.shape[0]
        self.total = int(self.lens.sum())
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        if k + "p0" in z.files:
            self.p0, self.g = z[k + "p0"], z[k + "g"]
        else:
            self.p0, self.g = seeded_inputs(int(z[k + "seed"]), self.total, self.steps)
            assert sha(self.p0) == str(z[k + "sha_p0"]) and sha(self.g) == str(z[k + "sha_g"]), "seeded inputs of %s drifted" % self.name
        self.sha_p, self.sha_m = [str(s) for s in z[k + "sha_p"]], [str(s) for s in z[k + "sha_m"]]
        self.born = z[k + "born"].astype(np.int32)
        self.p_final = z[k + "p_final"] if k + "p_final" in z.files else None
        self.m_final = z[k + "m_final"] if k + "m_final" in z.files else None

    def span(self, t):
        return slice(int(self.off[t]), int(self.off[t + 1]))


def load_cases(path):
    z = np.load(path, allow_pickle=False)
    return [Case(z, i) for i in range(int(z["n_cases"]))]


def run_reference(case):
    """The restatement over a whole case: lists over the steps of p [N], m [N] (zeros where unborn), born [T]."""
    p, m = case.p0.copy(), np.zeros(case.total, np.float32)
    born = np.zeros(len(case.lens), np.int32)
    out_p, out_m, out_b = [], [], []
    for s in range(case.steps):
        for t in range(len(case.lens)):
            sl = case.span(t)
            lr, mu, wd = case.hyper[s, case.group[t]]
            p[sl], m[sl], born[t] = sgd_update(p[sl], case.g[s, sl], m[sl], born[t], lr, mu, wd)
        out_p.append(p.copy()), out_m.append(m.copy()), out_b.append(born.copy())
    return out_p, out_m, out_b
