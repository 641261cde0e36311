"""Plain numpy reference of the top-k sort (csrc/topk.hip), a host mirror of the sample sort's splitter sampling, and the inputs that
tests/test_gpu_topk_seams.py feeds it.  Nothing here touches a device.

The order contract (docs/PARITY.md, "top-k order contract"):
  * the sort key is the score's BIT pattern under the order-preserving map key32(): -inf < negatives < -0.0 < +0.0 < denormals < normals
    < +inf, a NaN with the sign bit clear above +inf, a NaN with the sign bit set below -inf; equal keys are visited in index order;
  * all_live (frcnn_argsort_desc, ops.nms / batched_nms): every entry is sorted by that total order;
  * proposal mode (frcnn_topk_sorted): only LIVE entries, score >= 0, are sorted and counted: -0.0 is live, no NaN is.

Host mirror: plan() / sample_positions() / bucket_sizes() restate ss_plan and ss_sample_body of csrc/topk_dev.h -- S evenly spaced
samples, the samples of rank q * stride (q = 1..255) among them are the splitters, bucket b holds the composite keys in
[split[b + 1], split[b]).  The device ranks bucket b when its first rank is below the output count; above 1024 keys it takes the
"unlucky sample" branch.  The builders below place the scores so that this happens, and bucket_sizes() proves it without a GPU."""
import functools

import numpy as np

BUCKETS = 256
MIN_N = 4096                  # below: the rank sort (no sampling)
LDS_KEYS = 1024               # a bucket up to this size is ranked in one pass


# ---------------------------------------------------------------------------------------------- the reference sort
def key32(scores):
    """uint32 keys whose unsigned order is the total order on float32 bit patterns: a set sign bit flips every bit, a clear one only
    sets the top bit."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    neg = (u >> np.uint32(31)).astype(bool)
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def live_mask(scores, all_live=False):
    s = np.ascontiguousarray(scores, dtype=np.float32)
    if all_live:
        return np.ones(s.shape, bool)
    with np.errstate(invalid="ignore"):
        return s >= np.float32(0.0)                       # NaN: False; -0.0: True


def topk(scores, K, all_live=False):
    """(idx int64 [n], n): the first n = min(K, n_live) live entries by (key descending, index ascending)."""
    s = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    idx = np.nonzero(live_mask(s, all_live))[0]
    k = key32(s[idx]).astype(np.int64)
    order = idx[np.lexsort((idx, -k))]
    n = int(min(int(K), len(order)))
    return order[:n].astype(np.int64), n


# ---------------------------------------------------------------------------------------------- host mirror of the sampling
def plan(N, K):
    """(S, stride): samples per sort and the rank distance of two splitters among them."""
    S = 512 if N < 65536 else 2048
    full = S // BUCKETS
    stride = -((-3 * int(K) * S) // (2 * (BUCKETS - 1) * int(N)))            # ceil(1.5 K S / (255 N))
    return S, max(1, min(full, stride))


def sample_positions(N, S):
    return (np.arange(S, dtype=np.int64) * int(N)) // S


def _composite(k32, idx):
    return (k32.astype(np.uint64) << np.uint64(32)) | (~idx.astype(np.uint32)).astype(np.uint64)


def sort_keys(scores, all_live=False):
    """the 32-bit keys the device sorts by: in proposal mode an entry that is not live carries the key of -1"""
    s = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    return key32(np.where(live_mask(s, all_live), s, np.float32(-1.0)))


def bucket_sizes(scores, K, all_live=False):
    """(sizes int64 [256], first_rank int64 [256], n_out): what the sample sort's partition counts for this input, and the output
    count min(K, n_live).  Bucket b is ranked by the device when first_rank[b] < n_out and sizes[b] > 0."""
    s = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    N = len(s)
    assert N >= MIN_N, "the rank sort draws no sample"
    S, stride = plan(N, K)
    k32 = sort_keys(s, all_live)
    pos = sample_positions(N, S)
    comp = _composite(k32, np.arange(N))
    by_rank = np.sort(comp[pos])[::-1]                                        # composite order = (key desc, position asc)
    split = by_rank[stride * np.arange(1, BUCKETS)]                           # splitters 1..255, descending
    # bucket = number of splitters strictly above the key
    bucket = (BUCKETS - 1) - np.searchsorted(split[::-1], comp, side="right")
    sizes = np.bincount(bucket, minlength=BUCKETS).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return sizes, first, int(min(int(K), int(live_mask(s, all_live).sum())))


def ranked(scores, K, all_live=False):
    """sizes of the buckets the device ranks, in bucket order"""
    sizes, first, n_out = bucket_sizes(scores, K, all_live)
    return sizes[(first < n_out) & (sizes > 0)]


# ---------------------------------------------------------------------------------------------- inputs
def rand_boxes(rng, n, lo=0.02, hi=0.6):
    c = rng.rand(n, 2) * 0.8 + 0.1
    wh = rng.rand(n, 2) * (hi - lo) + lo
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


def _is_sample(N, K):
    m = np.zeros(N, bool)
    m[sample_positions(N, plan(N, K)[0])] = True
    return m


def low_samples(N, K, seed=0):
    """every sampled position scores below every other one: all splitters lie at the bottom and bucket 0 holds about N - S keys.
    Returns (scores, boxes, may_die): may_die marks the entries a test may set to -1 without breaking the promise."""
    rng = np.random.RandomState(seed)
    smp = _is_sample(N, K)
    s = (0.5 + 0.5 * rng.rand(N)).astype(np.float32)
    s[smp] = (0.01 + 0.09 * rng.rand(int(smp.sum()))).astype(np.float32)
    return s, rand_boxes(rng, N), np.ones(N, bool)


def high_samples(N, K, seed=0):
    """the mirror image: every sampled position scores above every other one, bucket 255 holds about N - S keys and its first rank is
    255 * stride + 1 (the samples above it and the splitter itself), which is below every K the tests use"""
    rng = np.random.RandomState(seed)
    smp = _is_sample(N, K)
    s = (0.01 + 0.49 * rng.rand(N)).astype(np.float32)
    s[smp] = (0.9 + 0.1 * rng.rand(int(smp.sum()))).astype(np.float32)
    return s, rand_boxes(rng, N), ~smp


EXACT_BUCKETS = ((1, LDS_KEYS), (3, LDS_KEYS + 1))        # (bucket, keys in it): the last size of the one-pass form and the first of the other


def exact_1024_1025(N, K, seed=0):
    """The sample of rank r scores 1 - r / 4096 (S <= 2048: all in (0.5, 1]), so splitter q is the level 1 - q * stride / 4096 and bucket b
    holds `stride` samples.  1024 - stride further keys are placed strictly between the samples of rank stride and stride + 1 (bucket 1)
    and 1025 - stride between those of rank 3 * stride and 3 * stride + 1 (bucket 3); every other entry scores below 0.4, far below the
    lowest sample."""
    rng = np.random.RandomState(seed)
    S, stride = plan(N, K)
    pos = sample_positions(N, S)
    smp = np.zeros(N, bool)
    smp[pos] = True
    s = (0.01 + 0.39 * rng.rand(N)).astype(np.float32)
    s[pos] = (1.0 - rng.permutation(S) / 4096.0).astype(np.float32)          # the ranks are scattered over the sample positions
    free = rng.permutation(np.nonzero(~smp)[0])
    may_die = ~smp
    at = 0
    for b, total in EXACT_BUCKETS:
        n = total - stride
        where = free[at:at + n]
        at += n
        s[where] = (1.0 - (b * stride + 0.25 + 0.5 * rng.rand(n)) / 4096.0).astype(np.float32)
        may_die[where] = False
    assert at <= len(free)
    return s, rand_boxes(rng, N), may_die


def periodic(N, K, seed=0):
    """A score map that is periodic in the entry index with the period of the sampling, N / S entries: the triangle 1 - |2 phi - 1| of the
    phase phi = frac(i S / N), lowest where the samples are drawn.  Where S divides N this is a function of i mod (N / S) with N / S
    distinct values (heavy ties); elsewhere (20646, 70000) the integer period N // S would let the sample positions drift through every
    residue -- a representative sample -- so the phase keeps the exact period.  About N - 2 S entries score above every sample."""
    S = plan(N, K)[0]
    i = np.arange(N, dtype=np.int64)
    phi = ((i * S) % N) / float(N)
    s = (0.05 + 0.9 * (1.0 - np.abs(2.0 * phi - 1.0))).astype(np.float32)
    return s, rand_boxes(np.random.RandomState(seed), N), np.ones(N, bool)


BUILDERS = {"low_samples": low_samples, "high_samples": high_samples, "exact_1024_1025": exact_1024_1025, "periodic": periodic}
UNLUCKY_NK = ((4096, 4096), (8192, 8192), (20646, 12000), (65536, 65536), (70000, 4000))
UNLUCKY_CASES = tuple((b, n, k) for b in ("low_samples", "high_samples", "exact_1024_1025", "periodic") for n, k in UNLUCKY_NK) \
    + (("low_samples", 20646, 6000),)
RANDOM_CASE = ("random", 20646, 12000)                   # the child processes' control: no bucket above 1024


@functools.lru_cache(maxsize=None)
def unlucky_case(builder, N, K):
    """(scores for the all_live sort, scores for proposal mode, boxes): the proposal-mode copy has 10 % of the entries that may die set
    to -1.  Read-only arrays, built once per process."""
    if builder == "random":
        rng = np.random.RandomState(N + K)
        s, boxes, may_die = rng.rand(N).astype(np.float32), rand_boxes(rng, N), np.ones(N, bool)
    else:
        s, boxes, may_die = BUILDERS[builder](N, K, 0)
    dead = s.copy()
    dead[may_die & (np.random.RandomState(N ^ K ^ 0x5EED).rand(N) < 0.1)] = -1.0
    for a in (s, dead, boxes):
        a.setflags(write=False)
    return s, dead, boxes


def case_inputs(builder, N, K, all_live):
    """(scores, boxes, K of the call): the all_live sort returns all N entries, so its plan -- and with it the exact builder's levels -- is
    the one of K = N"""
    if all_live:
        K = N
    s, dead, boxes = unlucky_case(builder, N, K)
    return (s if all_live else dead), boxes, K


def case_scores(builder, N, K, all_live):
    return case_inputs(builder, N, K, all_live)[0]


def promised(builder, N, K, all_live):
    """What the device's bucket counts must show for this case: {bucket: exact size} for the exact builder, else the string 'big'
    (some ranked bucket above 1024 keys), or 'none' for the random control."""
    if builder == "exact_1024_1025":
        return dict(EXACT_BUCKETS)
    return "none" if builder == "random" else "big"


def check_promise(builder, N, K, all_live, sizes, first, n_out):
    sizes, first = np.asarray(sizes, np.int64), np.asarray(first, np.int64)
    is_ranked = (first < n_out) & (sizes > 0)
    want = promised(builder, N, K, all_live)
    if want == "none":
        assert sizes[is_ranked].max() <= LDS_KEYS, (builder, N, K, int(sizes[is_ranked].max()))
        return
    assert (sizes[is_ranked] > LDS_KEYS).any(), (builder, N, K, all_live, "no ranked bucket above 1024 keys", int(sizes[is_ranked].max()))
    if isinstance(want, dict):
        for b, total in want.items():
            assert is_ranked[b] and sizes[b] == total, (builder, N, K, all_live, b, int(sizes[b]), total)


# ---------------------------------------------------------------------------------------------- size seams with ties
SEAM_N = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 4095, 4096, 4097, 65535, 65536)
SEAM_INPUTS = ("all_equal", "runs64", "runs1024", "ascending", "descending", "twelve_values")


def seam_scores(kind, N):
    i = np.arange(N)
    if kind == "all_equal":
        return np.full(N, 0.5, np.float32)
    if kind in ("runs64", "runs1024"):                    # two values in runs: equal keys on both sides of every chunk / block / segment border
        run = 64 if kind == "runs64" else 1024
        return np.where((i // run) % 2 == 0, np.float32(0.25), np.float32(0.75)).astype(np.float32)
    if kind == "ascending":
        return ((i + 1) / np.float32(N + 1)).astype(np.float32)
    if kind == "descending":
        return ((N - i) / np.float32(N + 1)).astype(np.float32)
    assert kind == "twelve_values"
    return (np.random.RandomState(N).randint(0, 12, N) / np.float32(16.0)).astype(np.float32)


def seam_dead(N):
    return (np.arange(N) % 7) == 3                        # proposal mode: every seventh entry is filtered


# ---------------------------------------------------------------------------------------------- special scores
def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


FLT_MAX, FLT_MIN = np.finfo(np.float32).max, np.finfo(np.float32).tiny
NAN_BITS = (0x7FC00000, 0x7F800001, 0xFFC00000, 0xFF800001)          # quiet / lowest signalling payload, sign clear and sign set
LIVE_SPECIALS = np.array([np.inf, FLT_MAX, 1.0, 0.5, FLT_MIN, 1e-40, 1e-45, 0.0], np.float32)
LIVE_SPECIALS = np.concatenate([LIVE_SPECIALS, _f([0x80000000])])                               # -0.0: live, after +0.0
NEG_SPECIALS = np.array([-np.inf, -FLT_MAX, -1.0, -0.5, -FLT_MIN, -1e-40, -1e-45], np.float32)


def special_scores(N, with_nan, seed=0):
    """Every special value many times over, drawn per entry, so equal keys lie on both sides of every 64 / 256 / 1024 border.  with_nan:
    five NaNs of each of the four bit patterns on top, index 0 and N - 1 among them."""
    rng = np.random.RandomState(seed + N)
    pool = np.concatenate([LIVE_SPECIALS, NEG_SPECIALS])
    s = pool[rng.randint(0, len(pool), N)].copy()
    if with_nan:
        u = s.view(np.uint32)
        where = np.concatenate([[0, N - 1], rng.choice(np.arange(1, N - 1), 5 * len(NAN_BITS) - 2, replace=False)])
        u[where] = np.repeat(np.array(NAN_BITS, np.uint32), 5)[rng.permutation(len(where))]
    return s


# ---------------------------------------------------------------------------------------------- the whole proposal stage
def proposal_logits(N, K, which, seed=0):
    """(reg, cls) of an RPN whose objectness at the sampled anchors is the lowest ('low') or the highest ('high') in the map; a few
    anchors that are not sampled collapse below min_size."""
    rng = np.random.RandomState(seed)
    smp = _is_sample(N, K)
    reg = (rng.randn(N, 4) * np.array([0.1, 0.1, 0.2, 0.2])).astype(np.float32)
    collapse = np.zeros(N, bool)
    collapse[::97] = True
    reg[collapse & ~smp, 2:] = -12.0
    d = (rng.rand(N) * 3.0 - 1.0).astype(np.float32)                                            # objectness logit in [-1, 2)
    d[smp] = ((-5.0 if which == "low" else 5.0) + rng.rand(int(smp.sum()))).astype(np.float32)
    return reg, np.stack([np.zeros(N, np.float32), d], 1)
