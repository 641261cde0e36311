"""The weight average of csrc/ema.hip restated in numpy, and the reader of tests/golden/ema.npz (written by tests/golden/make_golden_ema.py
from torch on the CPU: torch._foreach_lerp_, and torch.optim.swa_utils.AveragedModel over a torch.optim.SGD run).

    d  = round(p - e)
    e' = fma(w, d, e) if |w| < 0.5 else fma(round(w - 1), d, p)                     one rounding per fma (sgd_ref.fma32)
    decay_t = min(decay, (1 + n) / (10 + n)) under warm-up else decay, in binary64;  w = float32(1 - decay_t)

and the bookkeeping of the state block: an update while swapped is refused, one under a set skip word is skipped, any other is applied
and moves n."""
import os

import numpy as np

from sgd_ref import bits, fma32  # noqa: F401  (bits is what the tests compare with)

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ema.npz")


def weight(decay, warmup, n):
    """float32 weight of update number n (n updates applied so far)."""
    return F32(1.0 - (min(decay, (1 + n) / (10 + n)) if warmup else decay))


def lerp(e, p, w):
    """One tensor, one update: e' for the average e, the parameter p and the float32 weight w."""
    e, p, w = np.asarray(e, F32), np.asarray(p, F32), F32(w)
    with np.errstate(all="ignore"):
        d = (p - e).astype(F32)
        if abs(w) < F32(0.5):
            return fma32(w, d, e)
        return fma32(F32(w - F32(1.0)), d, p)


class State(object):
    """The state block: decay, warmup, n (num_updates), swapped, skipped, refused."""

    def __init__(self, decay, warmup, n=0):
        self.decay, self.warmup, self.n = float(decay), bool(warmup), int(n)
        self.swapped = self.skipped = self.refused = 0

    @property
    def w(self):
        return weight(self.decay, self.warmup, self.n)

    def update(self, ps, es, skip=0):
        """The stand-alone update (or the averaging half of a fused step): new list of averages; the bookkeeping moves."""
        if self.swapped:
            self.refused += 1
            return [np.array(e, F32) for e in es]
        if skip:
            self.skipped += 1
            return [np.array(e, F32) for e in es]
        w = self.w
        self.n += 1
        return [lerp(e, p, w) for p, e in zip(ps, es)]

    def swap(self):
        self.swapped ^= 1

    def stats(self):
        return dict(decay=self.decay, num_updates=self.n, w=float(self.w), warmup=self.warmup, swapped=self.swapped, skipped=self.skipped,
                    refused=self.refused)


def load():
    return np.load(GOLDEN, allow_pickle=False)


def trajectories(z):
    """[(name, decay, warmup, p [S, N], e0 [N], e [S, N], w [S])] of the fixture's _foreach_lerp_ trajectories."""
    out = []
    for i in range(int(z["n_traj"])):
        k = "t%d_" % i
        out.append((str(z[k + "name"]), float(z[k + "decay"]), bool(z[k + "warmup"]), z[k + "p"], z[k + "e0"], z[k + "e"], z[k + "w"]))
    return out
