"""The gradient norm of csrc/grad_norm.hip restated in numpy: the summation order include/frcnn_hip.h documents (chunk partials, finish),
then norm, clip coefficient, skip word and the counters of the state block.  Every addition is a binary64 addition in the documented
order; squares of binary32 values are exact in binary64.  Adding the +0 of an element that is not there changes nothing, so chunks and
trips are padded with zeros instead of being cut short.

    element   d = float64(x); d * d
    chunk     elements [8192 c, 8192 c + n) of a tensor; thread t = (i // 4) % 256 owns element i of the chunk, one accumulator per i % 4,
              squares added in increasing i; a = (a0 + a1) + (a2 + a3); xor butterfly (32, 16, .. 1) inside each wave of 64; the four
              waves in order
    finish    T = 1024 threads; thread t adds partials t, t + T, ...; butterfly inside each of the 16 waves; the waves in order"""
import numpy as np

CHUNK, THREADS, WAVE, FINISH_THREADS = 8192, 256, 64, 1024
CLIP, SKIP_NONFINITE = 1, 2
INT32_MAX = 2 ** 31 - 1
_LANE = np.arange(WAVE)


def n_chunks_of(numel):
    return (int(numel) + CHUNK - 1) // CHUNK


def butterfly(v):
    """v [..., 64] binary64: the xor butterfly; every lane ends with the same bits."""
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ d]
    return v


def chunk_partials(x):
    """x: one tensor, flat binary32.  Returns (partials [k] float64, counts [k] int32), k = ceil(numel / 8192)."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    k = n_chunks_of(x.size)
    if k == 0:
        return np.zeros(0, np.float64), np.zeros(0, np.int32)
    with np.errstate(all="ignore"):
        d = np.zeros(k * CHUNK, np.float64)
        d[:x.size] = x.astype(np.float64)
        sq = (d * d).reshape(k, CHUNK // (4 * THREADS), THREADS, 4)
        a = np.zeros((k, THREADS, 4), np.float64)
        for j in range(sq.shape[1]):
            a = a + sq[:, j]
        t = (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])
        w = butterfly(t.reshape(k, THREADS // WAVE, WAVE))[..., 0]
        part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    bad = np.zeros(k * CHUNK, bool)
    bad[:x.size] = ~np.isfinite(x)
    return part, bad.reshape(k, CHUNK).sum(1).astype(np.int32)


def finish(partials, counts, T=FINISH_THREADS):
    """(sumsq float64, non-finite count, saturated) from the partials and counts of every chunk in map order."""
    n = len(partials)
    trips = max(1, (n + T - 1) // T)
    p = np.zeros(trips * T, np.float64)
    p[:n] = partials
    with np.errstate(all="ignore"):
        s = np.zeros(T, np.float64)
        for r in p.reshape(trips, T):
            s = s + r
        w = butterfly(s.reshape(T // WAVE, WAVE))[:, 0]
        total = w[0]
        for v in w[1:]:
            total = total + v
    return np.float64(total), min(int(np.asarray(counts, np.int64).sum()), INT32_MAX)


def sumsq_of(tensors, T=FINISH_THREADS):
    parts = [chunk_partials(t) for t in tensors]
    return finish(np.concatenate([p for p, _ in parts]) if parts else np.zeros(0), np.concatenate([c for _, c in parts]) if parts else np.zeros(0, np.int32), T)


def additions_on_the_longest_path(numels, T=FINISH_THREADS):
    """D: the number of binary64 additions between a square and sumsq on the longest path, from the sizes alone.  In a chunk of n elements
    an accumulator takes ceil(n / 1024) squares at most, then 2 (the four accumulators), 6 (butterfly), 3 (waves); the finish adds
    ceil(n_chunks / T) partials per thread, then 6 and T / 64 - 1."""
    longest = max((min(CHUNK, int(n)) for n in numels), default=0)
    chunks = sum(n_chunks_of(n) for n in numels)
    in_chunk = (longest + 4 * THREADS - 1) // (4 * THREADS) + 2 + 6 + 3
    return in_chunk + (chunks + T - 1) // T + 6 + (T // WAVE - 1)


def state_after(tensors, max_norm, flags, user_guard=None, steps=0, skipped_steps=0, T=FINISH_THREADS):
    """The state block frcnn_grad_norm leaves: dict(sumsq, norm, coef, skip, nonfinite, steps, skipped_steps)."""
    sumsq, nonfinite = sumsq_of(tensors, T)
    with np.errstate(all="ignore"):
        norm = np.float32(np.sqrt(sumsq))
        coef = np.float32(1.0)
        if flags & CLIP:
            c = np.float32(max_norm) / (norm + np.float32(1e-6))
            coef = np.float32(1.0) if c > np.float32(1.0) else np.float32(c)
    skip = int(bool(flags & SKIP_NONFINITE and nonfinite != 0) or bool(user_guard))
    return dict(sumsq=sumsq, norm=norm, coef=coef, skip=skip, nonfinite=nonfinite, steps=steps + 1, skipped_steps=skipped_steps + skip)


def f64_bits(v):
    """The bit pattern of a binary64, every NaN as one pattern."""
    v = np.float64(v)
    return np.uint64(0x7FF8000000000000) if np.isnan(v) else np.array(v).view(np.uint64)[()]


def f32_bits(v):
    v = np.float32(v)
    return np.uint32(0x7FC00000) if np.isnan(v) else np.array(v).view(np.uint32)[()]
