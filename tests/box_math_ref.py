"""Case builders and plain float64 / exact references for the box arithmetic of csrc/frcnn_common.h (det_expf, det_log2f, decode4,
encode4, iou_pair, clamp01, the softmax and keep rule of prologue_one) and the FPN level mapper level_of (csrc/roi_align.hip).

Imports neither the oracle nor the library: the references below are numpy float64 (or exact by construction), the inputs are built
by bit pattern.  tests/test_box_math_host.py checks the premises on the CPU oracle, tests/test_gpu_box_math_seams.py the kernels.

Every bound that a test asserts is a constant of this file, with how it was measured and the input that attains it; the same figures
stand in docs/PARITY.md ("Box arithmetic").  The rule for a measured bound: the maximum over the input set, rounded up to the next
whole unit, plus one unit -- the set is a sample of the domain, not all of it.
"""
import functools
import math

import numpy as np

F32 = np.float32
HALF_ULP = 2.0 ** -24                      # relative error of one correctly rounded binary32 operation
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = 2.0 ** -126                      # smallest normal
DENORM = 2.0 ** -149                       # smallest subnormal = the unit of a subnormal result


# ============================================================================================ bit patterns
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(np.asarray(u, dtype=np.int64).astype(np.uint32)).view(np.float32)


def bits1(x):
    """Bit pattern of float32(x) as a Python int."""
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def ulp_window(x, n):
    """Every binary32 value within +-n ulps of float32(x) (x far enough from 0 that the window stays on its side)."""
    b = bits1(x)
    assert (b & 0x7FFFFFFF) > n
    return from_bits(np.arange(b - n, b + n + 1, dtype=np.int64))


def same_bits(got, want):
    """Equal in every bit; a NaN matches any NaN (the payload of a NaN that went through an arithmetic instruction is not pinned)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    n = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), n) and np.array_equal(bits(got)[~n], bits(want)[~n]))


def first_difference(got, want):
    """For a failure message: index, got, want of the first element that same_bits objects to."""
    got, want = np.ascontiguousarray(got, dtype=np.float32).ravel(), np.ascontiguousarray(want, dtype=np.float32).ravel()
    bad = np.nonzero(~(((bits(got) == bits(want)) & ~np.isnan(want)) | (np.isnan(got) & np.isnan(want))))[0]
    if not len(bad):
        return None
    i = int(bad[0])
    return i, float(got[i]), float(want[i]), len(bad)


def ulp32(v):
    """Spacing of binary32 at magnitude |v| (float64 in, float64 out); the subnormal spacing below 2^-126."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.frexp(np.maximum(v, FLT_MIN))[1]                  # v = m * 2^e, m in [0.5, 1)
    return np.ldexp(1.0, e - 24)


def is_dyadic(a, frac_bits):
    """All finite entries are multiples of 2^-frac_bits."""
    a = np.asarray(a, dtype=np.float64)
    f = a[np.isfinite(a)] * (2.0 ** frac_bits)
    return bool((f == np.rint(f)).all())


# ============================================================================================ 1. exp
EXP_HI = 88.72283935546875                 # det_expf: x > EXP_HI -> +inf
EXP_LO = -103.97283935546875               # det_expf: x < EXP_LO -> +0
LN2 = math.log(2.0)

# Measured on exp_inputs() (tests/test_box_math_host.py prints both): orc_expf against numpy's float64 exp.
#   normal results:    3.0054 ulp of the correctly rounded binary32 result, at x = -48.8668213 (bits 0xC24377A0)
#   subnormal results: 1.5701 units of 2^-149, at x = -87.6827164 (bits 0xC2AF5D8D)
# The truncation error of the degree-6 polynomial alone is r^7/5040 ~ 1.2e-7 relative at |r| = ln2/2, about 2 ulp at the top of a
# binade, so a bound under 3 would be wrong.  Asserted: the maximum rounded up to the next whole unit, plus one.
EXP_MEASURED_ULP = 3.0054
EXP_MEASURED_SUB = 1.5701
EXP_BOUND_ULP = 5.0
EXP_BOUND_SUB = 3.0


@functools.lru_cache(maxsize=None)
def exp_inputs():
    """Input set E of the exp tests, float32, read-only.  The cut-offs, the rounding seam of k at (k + 0.5) ln2 for every k that can
    occur (odd negative k included: k >> 1), the whole subnormal-result range densely, a 97-stepped walk over every magnitude from 2^-30
    to 104 in both signs, zeros / subnormals and the specials."""
    parts = []
    centers = [EXP_HI, EXP_LO, math.log(2.0 ** -126)] + [(k + 0.5) * LN2 for k in range(-151, 129)]
    for c in centers:
        parts.append(ulp_window(c, 64))
    parts.append(from_bits([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x80800000]))
    lo, hi = bits1(87.3), bits1(103.98)                       # results from 2^-126 down to below 2^-150
    parts.append(from_bits(np.arange(lo, hi + 1, 3, dtype=np.int64) | 0x80000000))
    walk = np.arange(bits1(2.0 ** -30), bits1(104.0) + 1, 97, dtype=np.int64)
    parts.append(from_bits(walk))
    parts.append(from_bits(walk | 0x80000000))
    parts.append(exp_specials())
    x = np.concatenate(parts)
    x.setflags(write=False)
    return x


def exp_specials():
    """quiet NaN, NaN with a payload, negative NaN, +-inf, +-FLT_MAX, 89, -104, -200"""
    return np.concatenate([from_bits([0x7FC00000, 0x7FC12345, 0xFFC00000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF]),
                           np.array([89.0, -104.0, -200.0], np.float32)])


def exp_as_decode_rows(x):
    """(t, anchors) with x in columns 2 and 3 of t and anchors (0, 0, 1, 1): decode returns exp(x) * 1.0 there, and * 1.0 is exact."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if len(x) % 2:
        x = np.concatenate([x, np.zeros(1, np.float32)])
    t = np.zeros((len(x) // 2, 4), np.float32)
    t[:, 2], t[:, 3] = x[0::2], x[1::2]
    a = np.tile(np.array([0, 0, 1, 1], np.float32), (len(t), 1))
    return t, a


def exp_from_decode(out, n):
    out = np.ascontiguousarray(out, dtype=np.float32)
    return np.ascontiguousarray(out[:, 2:4]).reshape(-1)[:n]


def exp_errors(x, got):
    """Error of got = exp(x) against numpy's float64 exp for every finite x <= EXP_HI: in ulps of the correctly rounded binary32
    result where the true result is normal, in units of 2^-149 where it is subnormal.  Where the correctly rounded result is +inf (only
    x = EXP_HI itself: its exp is 2^128 * (1 + 2.4e-7)) a got of +inf is no error, and a finite got is measured in ulps of the top binade.
    Returns (err [n] float64, normal [n] bool, measured [n] bool)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x64 = x.astype(np.float64)
    measured = ~np.isnan(x) & (x64 <= EXP_HI)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want = np.exp(np.where(measured, x64, 0.0))
        normal = want >= FLT_MIN
        c = np.minimum(want.astype(np.float32).astype(np.float64), 2.0 ** 128)   # correctly rounded (double rounding: see PARITY.md)
        unit = np.where(normal, ulp32(np.minimum(c, FLT_MAX)), DENORM)
        g = np.minimum(np.ascontiguousarray(got, dtype=np.float32).astype(np.float64), 2.0 ** 128)
        err = np.where(measured, np.abs(g - want) / unit, 0.0)
        err = np.where(np.isinf(want.astype(np.float32)) & (g == 2.0 ** 128), 0.0, err)
    return err, normal & measured, measured


def exp_maxima(x, got):
    """((max ulp, x), (max subnormal units, x)) of exp_errors."""
    err, normal, measured = exp_errors(x, got)
    out = []
    for m in (normal, measured & ~normal):
        e = np.where(m, err, -1.0)
        i = int(np.argmax(e))
        out.append((float(e[i]), float(x[i])))
    return tuple(out)


# ============================================================================================ 2. log2 and the level mapper
SQRT2_CUT = 1.41421353816986083984375      # det_log2f folds m > SQRT2_CUT into [0.707, 1.414]

# Error unit of det_log2f: 2^-22 (one binary32 ulp of a result in [2, 4)) while |log2 a| < 4 -- that is an ABSOLUTE error there, which
# is what the level mapper needs -- and one ulp of the result beyond.
# Measured on log2_inputs() (orc_log2f against numpy's float64 log2; the host test prints both):
#   a in [1/16, 16]:  2.1305e-07 absolute = 0.8936 units, at a = 0.0868404 (bits 0x3DB1D963)
#   every exponent:   0.6541 units, at a = 5.7150517 (bits 0x40B6E1B4); beyond |log2 a| = 4 the maximum is 0.5828 ulp of the result
# Asserted: rounded up to one whole unit, plus one.
LOG2_MEASURED_ABS = 2.1305e-07
LOG2_MEASURED_UNITS = 0.8936
LOG2_BOUND_UNITS = 2.0


def log2_unit(want):
    w = np.abs(np.asarray(want, dtype=np.float64))
    return np.where(w < 4.0, 2.0 ** -22, ulp32(w))


@functools.lru_cache(maxsize=None)
def log2_inputs():
    """(narrow, wide): narrow = stratified sample of [1/16, 16] (every 37th mantissa of each binade, 1 +- 4096 ulps, the fold point
    sqrt(2) +- 64 ulps in every binade, the binade ends); wide = 64 random mantissas in every binade of binary32 plus a walk over the
    subnormals."""
    rng = np.random.RandomState(20240)
    parts = []
    for e in range(-4, 4):
        b0 = (e + 127) << 23
        parts.append(from_bits(b0 + np.arange(0, 1 << 23, 37, dtype=np.int64)))
        parts.append(ulp_window(SQRT2_CUT * 2.0 ** e, 64))
        parts.append(ulp_window(2.0 ** e, 64))
    parts.append(ulp_window(1.0, 4096))
    parts.append(np.array([16.0], np.float32))
    narrow = np.concatenate(parts)
    narrow = narrow[(narrow >= 1 / 16) & (narrow <= 16)]
    wide = [from_bits(((e << 23) + rng.randint(0, 1 << 23, 64)).astype(np.int64)) for e in range(1, 255)]
    wide.append(from_bits(np.arange(1, 1 << 23, 4099, dtype=np.int64)))
    wide.append(from_bits([0x007FFFFF, 0x00800000, 0x7F7FFFFF]))
    wide = np.concatenate(wide)
    narrow.setflags(write=False)
    wide.setflags(write=False)
    return narrow, wide


def log2_errors(a, got):
    """|got - log2(a)| in float64, and the same in log2_unit()s."""
    want = np.log2(np.ascontiguousarray(a, dtype=np.float32).astype(np.float64))
    err = np.abs(np.ascontiguousarray(got, dtype=np.float32).astype(np.float64) - want)
    return err, err / log2_unit(want)


def powers_of_two():
    """(a, exact log2) for 2^-149 .. 2^127: the subnormal branch (e = -24 offset) and every normal exponent."""
    e = np.arange(-149, 128)
    return np.ldexp(1.0, e).astype(np.float32), e.astype(np.float32)


LEVEL_PARAMS = ((2, 5, 224.0, 4, 1e-6),    # torchvision's defaults as the RoI head uses them
                (0, 7, 56.0, 4, 0.0))      # wider clamp, other canonical size, eps = 0
LEVEL_OLD_SQUARES = (50, 111.9, 112, 223.9, 224, 447.9, 448, 895, 896, 2000, 0)


@functools.lru_cache(maxsize=None)
def level_rois():
    """Input set L, float32 [R, 4] xyxy in pixels, read-only; the last len(level_degenerate()) rows are the degenerate ones."""
    rng = np.random.RandomState(4)
    parts = []
    for side in (112.0, 224.0, 448.0):                                   # sqrt(area) on a level boundary +- 200 ulps
        s = ulp_window(side, 200)
        parts.append(np.stack([np.zeros_like(s), np.zeros_like(s), s, s], 1))
    for j in (-1, 0, 1):                                                 # rectangles of area (224 * 2^j)^2 * (1 + delta) at random offsets
        n = 20000
        w = rng.uniform(20.0, 1200.0, n)
        delta = rng.uniform(-3e-6, 3e-6, n)
        h = (224.0 * 2.0 ** j) ** 2 / w * (1.0 + delta)
        x1, y1 = rng.uniform(0.0, 300.0, n), rng.uniform(0.0, 300.0, n)
        parts.append(np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32))
    parts.append(np.array([[0, 0, s, s] for s in LEVEL_OLD_SQUARES], np.float32))
    for side in (3.5, 7.0, 14.0, 28.0, 56.0):                             # the lower boundaries of the second parameter set; all k_min for the first
        s = ulp_window(side, 8)
        parts.append(np.stack([np.zeros_like(s), np.zeros_like(s), s, s], 1))
    parts.append(np.array([r for _, r, _ in level_degenerate()], np.float32))
    rois = np.concatenate(parts)
    rois.setflags(write=False)
    return rois


def level_degenerate():
    """(name, roi, which end of the clamp the level must be).  sqrt of a negative area is NaN, NaN never passes k >= k_min."""
    inf, nan = float("inf"), float("nan")
    return [("zero area", [10, 10, 10, 50], "min"),
            ("zero area, both sides", [7, 7, 7, 7], "min"),
            ("negative zero area", [1, 0, 0.5, 0], "min"),
            ("negative width", [50, 10, 20, 300], "min"),
            ("negative width and height: positive area", [300, 300, 0, 76], None),       # (-300) * (-224): an ordinary row
            ("NaN coordinate", [0, nan, 200, 200], "min"),
            ("NaN coordinate last", [0, 0, 200, nan], "min"),
            ("inf coordinate", [0, 0, inf, 200], "max"),
            ("inf minus inf", [inf, 0, inf, 200], "min"),
            ("subnormal area", [0, 0, 2.0 ** -70, 2.0 ** -70], "min"),
            ("smallest subnormal area", [0, 0, 2.0 ** -75, 2.0 ** -74], "min"),
            ("area overflows to inf", [0, 0, 2.0 ** 70, 2.0 ** 70], "max")]


def level_reference(rois, k_min, k_max, s0, k0, eps):
    """Allowed levels (lo, hi, both inclusive, already minus k_min) of every row, and band, t64.

    t64 = k0 + log2(sqrt(area) / s0) + eps in float64 from the binary32 coordinates (eps = the binary32 value the kernel adds).  The
    kernel's t differs from t64 by at most `band`, derived from its chain of binary32 operations, each correctly rounded, relative error
    at most u = 2^-24:
        w = x2 - x1, h = y2 - y1        u each
        area = w * h                    u          -> area is off by 3u (relative)
        s = sqrt(area)                  halves what comes in, adds u   -> 2.5u
        q = s / s0                      u          -> 3.5u; s0 is a binary32 value, no error of its own
        log2(q)                         a relative error d of q moves log2 by d / ln2   -> 3.5u / ln2 = 3.01e-7
        det_log2f's own error           LOG2_BOUND_UNITS * log2_unit(L), asserted on the oracle by the host test (4.77e-7 for |L| < 4)
        t1 = k0 + L                     half an ulp at |t1| (2.38e-7 for t1 in [4, 8))
        t  = t1 + eps                   half an ulp at |t|
    (second-order terms: a factor 1 + 1e-6 on the relative part; the ulps are taken one band further out so that a binade edge between
    t64 and t cannot make them too small).  For t in [4, 8) and |L| < 4 this is 1.26e-6.
    If t64 is farther than band from every integer, floor(t) = floor(t64) and the level is clip(floor(t64)); otherwise it is one of the
    two levels on either side of that integer.
    Rows outside the chain's premises are decided by saturation, exactly: area NaN or negative -> sqrt is NaN -> k_min; area +-0 ->
    log2 is -inf -> k_min; area +inf in binary32 -> k_max; area below 2^-126 (subnormal: the product's relative error is unbounded,
    but s < 2^-62) -> k_min.
    """
    r = np.ascontiguousarray(rois, dtype=np.float32).astype(np.float64)
    eps64 = float(np.float32(eps))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w, h = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
        area = w * h
        to_min = np.isnan(area) | (area <= 0.0) | (area < FLT_MIN)
        to_max = ~to_min & (area > FLT_MAX)
        chain = ~to_min & ~to_max
        a = np.where(chain, area, 1.0)
        L = np.log2(np.sqrt(a) / s0)
        t1 = k0 + L
        t64 = t1 + eps64
        band = 3.5 * HALF_ULP * (1.0 + 1e-6) / LN2 + LOG2_BOUND_UNITS * log2_unit(np.abs(L) + 1e-5) \
            + 0.5 * ulp32(np.abs(t1) + 1e-5) + 0.5 * ulp32(np.abs(t64) + 1e-5)
        near = np.rint(t64)
        decided = np.abs(t64 - near) > band
        lo = np.where(decided, np.floor(t64), near - 1.0)
        hi = np.where(decided, np.floor(t64), near)
    lo = np.where(to_min, k_min, np.where(to_max, k_max, lo))
    hi = np.where(to_min, k_min, np.where(to_max, k_max, hi))
    lo = np.clip(lo, k_min, k_max).astype(np.int32) - k_min
    hi = np.clip(hi, k_min, k_max).astype(np.int32) - k_min
    t64 = np.where(chain, t64, np.nan)
    return lo, hi, np.where(chain, band, 0.0), t64


# ============================================================================================ 3. IoU on exact data
IOU_SHAPES = ((1, 1), (65, 3), (777, 1), (300, 7))
IOU_EPS = 1e-5


def iou_named():
    """(name, p, q, iou without eps or None, iou with eps 1e-5 is 0 / not): pairs in multiples of 2^-10.  The stated value is the
    hand-derived one; the full matrix of all names against all names is compared with iou_reference as well."""
    k = 1.0 / 1024
    inf, nan = float("inf"), float("nan")
    return [("identical", [0.25, 0.25, 0.75, 0.5], [0.25, 0.25, 0.75, 0.5], 1.0),
            ("sharing an edge", [0.0, 0.0, 0.5, 0.5], [0.5, 0.0, 1.0, 0.5], 0.0),
            ("sharing a corner", [0.0, 0.0, 0.5, 0.5], [0.5, 0.5, 1.0, 1.0], 0.0),
            ("disjoint", [0.0, 0.0, 100 * k, 100 * k], [0.5, 0.5, 0.75, 1.0], 0.0),
            ("nested", [0.0, 0.0, 1.0, 1.0], [0.25, 0.25, 0.75, 0.75], 0.25),
            ("one third", [0.0, 0.0, 0.5, 1.0], [0.25, 0.0, 0.75, 1.0], float(np.float32(1.0) / np.float32(3.0))),
            ("point in a box", [0.5, 0.5, 0.5, 0.5], [0.25, 0.25, 0.75, 0.75], 0.0),
            ("line in a box", [0.25, 0.5, 0.75, 0.5], [0.25, 0.25, 0.75, 0.75], 0.0),
            ("two identical empty boxes", [0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5], nan),              # 0/0; with eps 0/eps = 0
            ("inverted box, negative area", [0.75, 0.25, 0.25, 0.75], [0.0, 0.0, 1.0, 1.0], 0.0),         # union 1 - 1/4 = 3/4 > 0
            ("inverted both ways against itself", [0.75, 0.75, 0.25, 0.25], [0.75, 0.75, 0.25, 0.25], 0.0),
            ("negative union", [0.75, 0.0, 0.25, 1.0], [0.875, 0.0, 0.125, 1.0], -0.0),                   # 0 / (-1/2 - 3/4) = -0
            ("NaN in set 1", [0.25, nan, 0.75, 0.75], [0.0, 0.0, 1.0, 1.0], nan),
            ("NaN in set 2", [0.0, 0.0, 1.0, 1.0], [0.25, 0.25, nan, 0.75], nan),
            ("inf coordinate", [0.0, 0.0, inf, 1.0], [0.25, 0.25, 0.75, 0.75], 0.0),                      # finite / inf
            ("inf in both", [0.0, 0.0, inf, 1.0], [0.5, 0.0, inf, 1.0], nan),                             # union inf + inf - inf
            # tmax(+0, -0) is its SECOND operand, -0, and tmin(1/2, -0) = -0: the width is (-0) - (-0) = +0 and the IoU +0 / (1/2) = +0.
            # A maximum that orders the zeros (fmaxf: +0) gives the width (-0) - (+0) = -0, which w < 0 lets through, and the IoU -0.
            # This is the one observable difference between tmax and fmaxf in iou_pair: a NaN coordinate makes its box's area NaN, and
            # with it the union and the IoU, whichever maximum is used.
            ("signed zeros", [0.0, 0.0, 0.5, 1.0], [-0.0, 0.0, -0.0, 1.0], 0.0)]


def dyadic_boxes(rng, n, frac_bits=10, degenerate=0.1):
    """n xyxy boxes in [0, 1] with every coordinate a multiple of 2^-frac_bits; some points, lines and inverted boxes among them."""
    m = 1 << frac_bits
    a = np.sort(rng.randint(0, m + 1, (n, 2, 2)), axis=2)                # [n, xy, lo/hi]
    b = np.stack([a[:, 0, 0], a[:, 1, 0], a[:, 0, 1], a[:, 1, 1]], 1).astype(np.float64)
    flip = rng.rand(n) < degenerate / 2
    b[flip] = b[flip][:, [2, 1, 0, 3]]
    flat = rng.rand(n) < degenerate / 2
    b[flat, 3] = b[flat, 1]
    return (b / m).astype(np.float32)


@functools.lru_cache(maxsize=None)
def iou_sets(n1, n2):
    """The two sets of one shape: the named boxes (NaN and inf rows included) first as far as they fit, then random dyadic boxes."""
    rng = np.random.RandomState(1000 * n1 + n2)
    named = [(p, q) for _, p, q, _ in iou_named()]
    s1, s2 = dyadic_boxes(rng, n1), dyadic_boxes(rng, n2)
    for i in range(min(n1, len(named))):
        s1[i] = named[i][0]
    for j in range(min(n2, len(named))):
        s2[j] = named[j][1]
    s1.setflags(write=False)
    s2.setflags(write=False)
    return s1, s2


def tmax(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.where((a > b) | np.isnan(a), a, b)


def tmin(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.where((a < b) | np.isnan(a), a, b)


def iou_reference(s1, s2, eps):
    """(iou, union, inter) [n1, n2] binary32.  On coordinates that are multiples of 2^-10 in [0, 1] every difference, product and sum
    is an integer below 2^22 in units of 2^-20: exact in binary32 and in float64 alike.  The only roundings of the kernel are the add
    of eps (done here in binary32, on the exactly converted union) and the division; the float64 quotient rounded to binary32 is the
    correctly rounded binary32 quotient.  Double rounding cannot bite: numerator and denominator have at most 24 significant bits, so a
    quotient that is not itself a binary32 midpoint lies at least 2^-24 * 2^-24 = 2^-48 (relative) away from every midpoint, and the
    float64 rounding moves it by 2^-53 at most.
    Maximum and minimum are tmax / tmin of frcnn_common.h restated: a if a > b or a is NaN, else b -- NaN goes through as through
    torch.max / torch.min, and of two zeros the second is taken.  A NaN width stays NaN under the clamp, as in torch.clamp."""
    p = np.ascontiguousarray(s1, dtype=np.float32).astype(np.float64)[:, None, :]
    q = np.ascontiguousarray(s2, dtype=np.float32).astype(np.float64)[None, :, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        lx, ly = tmax(p[..., 0], q[..., 0]), tmax(p[..., 1], q[..., 1])
        ux, uy = tmin(p[..., 2], q[..., 2]), tmin(p[..., 3], q[..., 3])
        w, h = ux - lx, uy - ly
        w = np.where(w < 0, 0.0, w)
        h = np.where(h < 0, 0.0, h)
        inter = w * h
        a1 = (p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1])
        a2 = (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
        union = a1 + a2 - inter
        den = union
        if eps != 0.0:
            den = (union.astype(np.float32) + np.float32(eps)).astype(np.float64)
        iou = (inter / den).astype(np.float32)
    return iou, union.astype(np.float32), inter.astype(np.float32)


# ============================================================================================ 4. codec and prologue on exact data
def witness_cxcy():
    """(t, anchor cxcywh, x without contraction, x with a fused multiply-add).  t.x * a.z = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a tie
    in binary32 and rounds to even, 1 + 2^-11; adding a.x = -1 gives 2^-11.  A fused multiply-add keeps the 2^-24."""
    v = 1.0 + 2.0 ** -12
    return (np.array([v, 0, 0, 0], np.float32), np.array([-1.0, 0.5, v, 0.5], np.float32), 2.0 ** -11, 2.0 ** -11 + 2.0 ** -24)


def witness_xyxy():
    """The same witness for the prologue: an xyxy anchor whose centre form is exactly witness_cxcy()'s (cx = -1, w = 1 + 2^-12).  The
    decoded box is (cx' - w/2, cx' + w/2) with w/2 = 1/2 + 2^-13: x1 clamps to 0, x2 = 1/2 + 2^-13 + cx' shows the 2^-24 (one ulp at 1/2).
    Returns (t, anchor, x2 without contraction, x2 with)."""
    t, a, x, xf = witness_cxcy()
    hw = float(a[2]) / 2
    anchor = np.array([-1.0 - hw, 0.25, -1.0 + hw, 0.75], np.float32)
    assert float(anchor[2]) - float(anchor[0]) == float(a[2]) and (float(anchor[2]) + float(anchor[0])) / 2 == -1.0
    return t, anchor, x + hw, xf + hw


@functools.lru_cache(maxsize=None)
def decode_exact_case(n=777):
    """(t, anchors cxcywh): t.x, t.y multiples of 2^-8 in [-4, 4], t.z = t.w = 0; anchor centres multiples of 2^-10 in [-1, 2], sizes
    multiples of 2^-8 in (0, 1].  The product has at most 19 significant bits and the sum at most 21: nothing rounds.  Row 0 is the
    contraction witness, the one row on which the product does round."""
    rng = np.random.RandomState(8)
    t = np.zeros((n, 4), np.float64)
    t[:, :2] = rng.randint(-1024, 1025, (n, 2)) / 256.0
    a = np.empty((n, 4), np.float64)
    a[:, :2] = rng.randint(-1024, 2049, (n, 2)) / 1024.0
    a[:, 2:] = rng.randint(1, 257, (n, 2)) / 256.0
    t, a = t.astype(np.float32), a.astype(np.float32)
    t[0], a[0] = witness_cxcy()[:2]
    t.setflags(write=False)
    a.setflags(write=False)
    return t, a


def decode_reference(t, a):
    """decode with every operation rounded once to binary32, from float64 (the product of two binary32 values is exact in float64; the
    sum of two binary32 values of these magnitudes is too), and exp restricted to the arguments whose value is exact by definition."""
    t, a = np.asarray(t, np.float32), np.asarray(a, np.float32)
    t64, a64 = t.astype(np.float64), a.astype(np.float64)
    out = np.empty(t.shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in (0, 1):
            prod = (t64[:, c] * a64[:, 2 + c]).astype(np.float32).astype(np.float64)
            out[:, c] = (prod + a64[:, c]).astype(np.float32)
        for c in (2, 3):
            out[:, c] = (exact_exp(t64[:, c]) * a64[:, c]).astype(np.float32)
    return out


def exact_exp(z):
    """exp on {0, +inf, -inf, NaN} only: 1, +inf, 0, NaN."""
    z = np.asarray(z, np.float64)
    assert (np.isnan(z) | np.isinf(z) | (z == 0)).all(), "the exact-data cases keep t.z, t.w to 0, +-inf and NaN"
    return np.where(np.isnan(z), np.nan, np.where(z == 0, 1.0, np.where(z > 0, np.inf, 0.0)))


@functools.lru_cache(maxsize=None)
def encode_exact_case(n=777):
    """(g, a) in cxcywh: centres multiples of 2^-10 in [-1, 2], a.z / a.w powers of two or small odd multiples of 2^-8, g.z = a.z
    (log of exactly 1 is exactly 0).  The last rows divide by a.z = 0: x/0 and 0/0."""
    rng = np.random.RandomState(9)
    g = np.empty((n, 4), np.float64)
    a = np.empty((n, 4), np.float64)
    g[:, :2] = rng.randint(-1024, 2049, (n, 2)) / 1024.0
    a[:, :2] = rng.randint(-1024, 2049, (n, 2)) / 1024.0
    a[:, 2:] = rng.randint(1, 257, (n, 2)) / 256.0
    g[:, 2:] = a[:, 2:]
    a[-4:, 2] = 0.0
    g[-4:, 0] = a[-4:, 0] + np.array([0.5, -0.5, 0.0, 0.0])            # +inf, -inf, NaN, NaN
    g, a = g.astype(np.float32), a.astype(np.float32)
    g.setflags(write=False)
    a.setflags(write=False)
    return g, a


def encode_xy_reference(g, a):
    """Columns 0, 1 of encode: the difference is exact on dyadic data, the float64 quotient rounded to binary32 is the correctly
    rounded binary32 quotient (operands of at most 24 bits: the double-rounding argument of iou_reference), and division by zero follows
    IEEE in float64 as in binary32."""
    g64, a64 = np.asarray(g, np.float32).astype(np.float64), np.asarray(a, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((g64[:, :2] - a64[:, :2]) / a64[:, 2:]).astype(np.float32)


# logf of encode4, measured against numpy's float64 log in ulps of the correctly rounded binary32 result, on encode_log_case():
#   host (the oracle calls the C library's logf):  0.5051 ulp at g.z = 0.9204695 (bits 0x3F6BA3E4)
#   device (HIP's logf on gfx950):                  1.8659 ulp at g.z = 3.18703879e+24 (bits 0x6828B86E); over the subnormal ratios alone
#                                                   1.1459 ulp at g.z = 2.33004265e-39
# The ROCm installation the figures were taken on ships no document with an ulp bound for logf (its share/ and include/ trees were
# searched), so each asserted bound is the measured maximum rounded up to the next whole ulp, plus one.
LOGF_MEASURED_HOST = 0.5051
LOGF_MEASURED_DEVICE = 1.8659
LOGF_BOUND_ULP_HOST = 2.0
LOGF_BOUND_ULP_DEVICE = 3.0


@functools.lru_cache(maxsize=None)
def encode_log_case():
    """(g, a, special): a = (0, 0, 1, 1) so g.z / a.z = g.z exactly; g.z, g.w = 32 random mantissas in every binade of (0, FLT_MAX],
    a walk over the subnormals, 1 +- 64 ulps, then the specials: 0 (-inf), -0 (-inf), negative (NaN), -subnormal (NaN), +inf, NaN."""
    rng = np.random.RandomState(10)
    v = [from_bits(((e << 23) + rng.randint(0, 1 << 23, 32)).astype(np.int64)) for e in range(1, 255)]
    v.append(from_bits(np.arange(1, 1 << 23, 8191, dtype=np.int64)))
    v.append(ulp_window(1.0, 64))
    v.append(from_bits([0x7F7FFFFF, 0x00800000, 0x007FFFFF, 0x00000001]))
    v = np.concatenate(v)
    sp = np.concatenate([np.array([0.0, -0.0, -1.5], np.float32), from_bits([0x80000001, 0x7F800000, 0x7FC00000, 0xFF800000])])
    if (len(v) + len(sp)) % 2:
        v = np.concatenate([v, np.ones(1, np.float32)])
    z = np.concatenate([v, sp])
    g = np.zeros((len(z) // 2, 4), np.float32)
    g[:, 2], g[:, 3] = z[0::2], z[1::2]
    a = np.tile(np.array([0, 0, 1, 1], np.float32), (len(g), 1))
    g.setflags(write=False)
    a.setflags(write=False)
    return g, a, len(sp)


def log_check(z, got):
    """(max error in ulps over positive finite z, the z that attains it, specials all right).  Specials: log(+-0) = -inf,
    log(negative) = NaN, log(+inf) = +inf, log(NaN) = NaN; log(1) = 0 exactly."""
    z = np.ascontiguousarray(z, np.float32).ravel()
    got = np.ascontiguousarray(got, np.float32).ravel()
    z64 = z.astype(np.float64)
    pos = np.isfinite(z) & (z > 0)
    want = np.log(np.where(pos, z64, 1.0))
    c = want.astype(np.float32).astype(np.float64)
    err = np.where(pos, np.abs(got.astype(np.float64) - want) / ulp32(np.where(c == 0, 1.0, c)), 0.0)
    i = int(np.argmax(err))
    ok = bool((got[z == 0] == -np.inf).all() and np.isnan(got[(z < 0) | np.isnan(z)]).all() and (got[z == np.inf] == np.inf).all()
              and (got[z == 1] == 0).all())
    return float(err[i]), float(z[i]), ok


# -------------------------------------------------------------------------------------------- prologue
MIN_SIZE = 2.0 ** -10
TINY = 2.0 ** -20


def prologue_box_cases():
    """(name, t, anchor xyxy, kept by the size rule).  Dyadic anchors, t.z = t.w = 0 unless the row is about a special delta.  With
    t = 0 the box is cxcy_to_xy(xy_to_cxcy(anchor)) = the anchor, exactly (sums and halves of dyadic numbers), then clamped to [0, 1]."""
    m, e = MIN_SIZE, TINY
    inf, nan = float("inf"), float("nan")
    z = [0, 0, 0, 0]
    return [("width exactly min_size", z, [0.25, 0.25, 0.25 + m, 0.75], True),
            ("width min_size - 2^-20", z, [0.25, 0.25, 0.25 + m - e, 0.75], False),
            ("height exactly min_size", z, [0.25, 0.5, 0.75, 0.5 + m], True),
            ("height min_size - 2^-20", z, [0.25, 0.5, 0.75, 0.5 + m - e], False),
            ("both exactly min_size", z, [0.5, 0.5, 0.5 + m, 0.5 + m], True),
            ("straddles 0, clamped width exactly min_size", z, [-0.25, 0.25, m, 0.75], True),
            ("straddles 0, clamped width below", z, [-0.25, 0.25, m - e, 0.75], False),
            ("straddles 1, clamped width exactly min_size", z, [1.0 - m, 0.25, 1.5, 0.75], True),
            ("straddles 1, clamped width below", z, [1.0 - m + e, 0.25, 1.5, 0.75], False),
            ("straddles 0 and 1 in y, clamped height 1", z, [0.25, -0.5, 0.75, 1.5], True),
            ("straddles 1 in y, clamped height exactly min_size", z, [0.25, 1.0 - m, 0.75, 2.0], True),
            ("straddles 0 in y, clamped height below", z, [0.25, -1.0, 0.75, m - e], False),
            ("shifted left by t.x = 64 widths, width still exactly min_size", [-64.0, 0, 0, 0], [0.25 + m, 0.25, 0.25 + 2 * m, 0.75], True),
            ("contraction witness", list(witness_xyxy()[0]), list(witness_xyxy()[1]), True),
            ("NaN t.x", [nan, 0, 0, 0], [0.25, 0.25, 0.75, 0.75], False),
            ("NaN t.y", [0, nan, 0, 0], [0.25, 0.25, 0.75, 0.75], False),
            ("+inf t.x: both edges clamp to 1", [inf, 0, 0, 0], [0.25, 0.25, 0.75, 0.75], False),
            ("-inf t.y: both edges clamp to 0", [0, -inf, 0, 0], [0.25, 0.25, 0.75, 0.75], False),
            ("NaN t.z", [0, 0, nan, 0], [0.25, 0.25, 0.75, 0.75], False),
            ("+inf t.z: infinite width clamps to [0, 1]", [0, 0, inf, 0], [0.25, 0.25, 0.75, 0.75], True),
            ("-inf t.w: zero height", [0, 0, 0, -inf], [0.25, 0.25, 0.75, 0.75], False)]


def prologue_logit_cases():
    """(c0, c1, expected score before the size rule; -1 = not a number >= 0, filtered).  The expected value is exact: exp(0) = 1,
    exp(-inf) = 0, and exp(-200) = 0 by det_expf's lower cut-off."""
    inf, nan = float("inf"), float("nan")
    return [(0.0, 0.0, 0.5), (3.25, 3.25, 0.5), (-77.0, -77.0, 0.5), (1e30, 1e30, 0.5),
            (0.0, -inf, 0.0),                  # a score of exactly 0 passes sc >= 0: kept, as in the reference (softmax, then the size filter alone)
            (-inf, 0.0, 1.0), (0.0, 200.0, 1.0), (200.0, 0.0, 0.0), (-3e38, 3e38, 1.0),
            (-inf, -inf, -1.0), (2.5, inf, -1.0), (inf, 2.5, -1.0), (inf, inf, -1.0),
            (nan, 0.0, -1.0), (0.0, nan, -1.0), (nan, nan, -1.0)]


@functools.lru_cache(maxsize=None)
def prologue_case(N):
    """(reg, cls, anchors xyxy): row i takes box case i % nb and logit pair (i // nb) % nl
    while the product lasts, then random dyadic boxes (sizes multiples of 2^-10, so on or above min_size unless clamped away) with the
    logit pairs in turn."""
    boxes, logits = prologue_box_cases(), prologue_logit_cases()
    nb, nl = len(boxes), len(logits)
    rng = np.random.RandomState(N)
    reg = np.zeros((N, 4), np.float32)
    cls = np.zeros((N, 2), np.float32)
    anc = np.zeros((N, 4), np.float32)
    for i in range(N):
        c0, c1, _ = logits[(i // nb) % nl]
        cls[i] = (c0, c1)
        if i < nb * nl:
            _, t, a, _ = boxes[i % nb]
            reg[i], anc[i] = t, a
        else:
            x1, y1 = rng.randint(-256, 1024, 2) / 1024.0
            w, h = rng.randint(0, 3, 2) / 1024.0 if i % 3 == 0 else rng.randint(1, 512, 2) / 1024.0
            anc[i] = (x1, y1, x1 + w, y1 + h)
            reg[i, :2] = rng.randint(-8, 9, 2) / 4.0
    for a in (reg, cls, anc):
        a.setflags(write=False)
    return reg, cls, anc


def prologue_reference(reg, cls, anchors, min_size):
    """(boxes [N,4] binary32, scores [N] binary32, valid count) of RegionProposal.forward up to the sort, in float64 on exact data:
    the caller's data must make every finite intermediate exact (asserted: every finite result converts to binary32 and back unchanged),
    the one rounding product of the contraction witness is rounded to binary32 as decode_reference does.  The score is looked up from
    prologue_logit_cases() by the logit pair, not computed."""
    reg, cls, anchors = (np.asarray(x, np.float32) for x in (reg, cls, anchors))
    a = anchors.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ca = np.stack([(a[:, 2] + a[:, 0]) / 2, (a[:, 3] + a[:, 1]) / 2, a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]], 1)
        assert np.array_equal(ca.astype(np.float32).astype(np.float64), ca, equal_nan=True)
        d = decode_reference(reg, ca.astype(np.float32)).astype(np.float64)
        hw, hh = d[:, 2] / 2, d[:, 3] / 2
        b = np.stack([d[:, 0] - hw, d[:, 1] - hh, d[:, 0] + hw, d[:, 1] + hh], 1)
        fin = np.isfinite(b)
        assert np.array_equal(b[fin].astype(np.float32).astype(np.float64), b[fin])
        b = np.where(b < 0, 0.0, np.where(b > 1, 1.0, b))                      # NaN stays NaN
        ws, hs = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        keep = (hs >= min_size) & (ws >= min_size)
    table = {}
    for c0, c1, s in prologue_logit_cases():
        table[(bits1(c0), bits1(c1))] = s
    sc = np.array([table[(int(u), int(v))] for u, v in bits(cls).reshape(-1, 2)], np.float64)
    sc = np.where(keep & (sc >= 0), sc, -1.0)
    return b.astype(np.float32), sc.astype(np.float32), int((sc >= 0).sum()), keep


@functools.lru_cache(maxsize=None)
def region_proposal_case():
    """16 x 16 x 9 anchors of a 256 x 256 image at stride 16: ordinary deltas and logits, with every logit pair of prologue_logit_cases()
    planted at 16 positions each.  (reg, cls, planted index list)."""
    rng = np.random.RandomState(12)
    N = 16 * 16 * 9
    reg = (rng.randn(N, 4) * np.array([0.1, 0.1, 0.2, 0.2])).astype(np.float32)
    cls = np.stack([np.zeros(N, np.float32), (rng.randn(N) * 2 - 1).astype(np.float32)], 1)
    logits = prologue_logit_cases()
    where = rng.permutation(N)[:16 * len(logits)]
    for j, i in enumerate(where):
        cls[i] = logits[j % len(logits)][:2]
    reg.setflags(write=False)
    cls.setflags(write=False)
    return reg, cls, np.sort(where)
