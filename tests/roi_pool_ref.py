"""A numpy restatement of RoIPool (torchvision.ops.roi_pool: forward with argmax, backward as a float64 scatter), the named cases that
tests/test_roi_pool_ref_host.py proves on the CPU and tests/test_gpu_roi_pool_exact.py runs against the HIP kernels, and the censuses
that show from the reference alone that a case is not degenerate.

Nothing here is fitted to kernel output.  The geometry goes step by step in float32, in the order torchvision and csrc/roi_pool.hip
roi_bins() use:
    cell   = round half away from zero of fl32(coord * scale)
    side r = max(end - start + 1, 1)
    bin  b = fl32(fl32(r) / fl32(P))
    bin k  = [floor(fl32(fl32(k) * b)), ceil(fl32(fl32(k + 1) * b))) + start, clamped to [0, n]
The window is scanned row-major with a strict `>` from -FLT_MAX: the first of equal maxima wins (0.0 and -0.0 are equal: the first keeps
its sign), a NaN never wins, a window with nothing above -FLT_MAX (all NaN, all -inf) gives -FLT_MAX with argmax -1, an empty window 0
with argmax -1.  A maximum is exact on any data, so the forward is compared on arbitrary floats.

The backward is np.bincount with float64 weights.  With integer dOut in [-8, 8] and |sum| < 2^24 every partial sum of every order of
additions is an fp32 number: the kernels must return float32(ref64) in every bit, whatever their copies, ranks or atomics do.
"""
import functools

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max


# ---------------------------------------------------------------------------------------------- the three roundings
def round_half_away(x):
    """C roundf().  x - trunc(x) is exact, so nothing is rounded twice (floor(x + 0.5) is wrong at 0.49999997)."""
    x = np.asarray(x)
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0).astype(x.dtype)


def round_half_even(x):
    return np.rint(np.asarray(x))


def round_floor_half(x):
    x = np.asarray(x)
    return np.floor(x + x.dtype.type(0.5))


# ---------------------------------------------------------------------------------------------- geometry
def bin_edges(start, r, P):
    """(lo, hi) int64 [P]: the P bins of a side of r cells beginning at `start`, not yet clamped.  float32 step by step."""
    b = F(r) / F(P)
    k = np.arange(P, dtype=F)
    lo, hi = np.floor(k * b), np.ceil((k + F(1)) * b)
    assert type(b) is F and lo.dtype == F and hi.dtype == F
    return lo.astype(np.int64) + start, hi.astype(np.int64) + start


def roi_cells(roi, scale, rounding=round_half_away, product=F):
    """(sw, sh, ew, eh): the cells of the box's corners.  product: the type the multiplication by the scale is done (and rounded) in."""
    p = np.asarray(roi, F).astype(product) * product(F(scale))             # the scale is a float32 argument
    assert p.dtype == product
    return tuple(int(v) for v in rounding(p))


def roi_windows(roi, scale, PH, PW, H, W, rounding=round_half_away, product=F):
    """(hs, he, ws, we, raw): clamped bin boundaries (int64 [PH], [PH], [PW], [PW]); raw = the same four before the clamp."""
    sw, sh, ew, eh = roi_cells(roi, scale, rounding, product)
    rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
    hs, he = bin_edges(sh, rh, PH)
    ws, we = bin_edges(sw, rw, PW)
    raw = (hs, he, ws, we)
    return np.clip(hs, 0, H), np.clip(he, 0, H), np.clip(ws, 0, W), np.clip(we, 0, W), raw


# ---------------------------------------------------------------------------------------------- forward
def fwd(feat, rois, PH=7, PW=7, scale=1.0, rounding=round_half_away, product=F):
    """feat [C, H, W], rois [R, 4] -> (out float32 [R, C, PH, PW], argmax int32, -1 = no pixel).  One numpy call chain per (RoI, bin)."""
    feat = np.ascontiguousarray(feat, F)
    rois = np.asarray(rois, F).reshape(-1, 4)
    C, H, W = feat.shape
    R = rois.shape[0]
    out = np.zeros((R, C, PH, PW), F)
    arg = np.full((R, C, PH, PW), -1, np.int32)
    ch = np.arange(C)
    for r in range(R):
        hs, he, ws, we, _ = roi_windows(rois[r], scale, PH, PW, H, W, rounding, product)
        for ph in range(PH):
            if he[ph] <= hs[ph]:
                continue
            for pw in range(PW):
                ww = int(we[pw] - ws[pw])
                if ww <= 0:
                    continue
                win = feat[:, hs[ph]:he[ph], ws[pw]:we[pw]].reshape(C, -1)
                cand = win > -FLT_MAX                                   # False for a NaN, for -inf and for -FLT_MAX itself
                i = np.where(cand, win, -np.inf).argmax(axis=1)         # the FIRST of equal maxima, row-major
                has = cand[ch, i]
                out[r, :, ph, pw] = np.where(has, win[ch, i], -FLT_MAX)
                arg[r, :, ph, pw] = np.where(has, (hs[ph] + i // ww) * W + ws[pw] + i % ww, -1)
    return out, arg


# ---------------------------------------------------------------------------------------------- backward
def bwd64(go, arg, C, H, W):
    """float64 scatter -> (grad [C, H, W] float64, n = terms per pixel (int64), mag = sum of |term| per pixel (float64))."""
    R = arg.shape[0]
    a = arg.reshape(R, C, -1).astype(np.int64)
    live = a >= 0
    flat = (np.arange(C)[None, :, None] * (H * W) + a)[live]
    g = np.asarray(go).reshape(R, C, -1).astype(np.float64)[live]
    grad = np.bincount(flat, weights=g, minlength=C * H * W).reshape(C, H, W) + 0.0
    n = np.bincount(flat, minlength=C * H * W).reshape(C, H, W)
    mag = np.bincount(flat, weights=np.abs(g), minlength=C * H * W).reshape(C, H, W)
    return grad, n, mag


def gamma(m):
    """m u / (1 - m u), u = 2^-24: |fl(sum) - sum| <= gamma(n - 1) * sum |terms| for ANY order of n fp32 additions (Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2: each term passes through at most n - 1 roundings, whatever the tree)."""
    m = np.asarray(m, np.float64)
    u = 2.0 ** -24
    return m * u / (1.0 - m * u)


def a16(arg):
    """int32 argmax -> the 16-bit pair's encoding (0xFFFF = -1)."""
    assert arg.max() < 0xFFFF
    return np.where(arg < 0, 0xFFFF, arg).astype(np.uint16)


# ---------------------------------------------------------------------------------------------- cases
class Case(object):
    def __init__(self, name, feat, rois, scale=1.0, **notes):
        self.name, self.feat, self.rois, self.scale = name, np.ascontiguousarray(feat, F), np.ascontiguousarray(rois, F).reshape(-1, 4), float(scale)
        self.C, self.H, self.W = self.feat.shape
        self.R = self.rois.shape[0]
        self.notes = notes

    def go(self, PH=7, PW=7):
        """integer dOut in [-8, 8]"""
        rng = np.random.RandomState(self.R * 31 + self.C * 7 + PH)
        return rng.randint(-8, 9, (self.R, self.C, PH, PW)).astype(F)

    def go_float(self):
        return np.random.RandomState(self.R * 17 + self.C).randn(self.R, self.C, 7, 7).astype(F)


def distinct_planes(rng, C, H, W):
    """every channel a random permutation of H * W distinct values around zero"""
    return (rng.rand(C, H * W).argsort(axis=1).astype(F) - F(H * W // 2)).reshape(C, H, W)


GEO_HW = (16, 60)
HALVES = np.array([[0.5, 0.5, 2.5, 2.5], [1.5, 2.5, 9.5, 8.5], [-0.5, -1.5, 6.5, 7.5], [2.5, 0.5, 12.5, 10.5], [-2.5, -0.5, 10.5, 12.5],
                   [20.5, 3.5, 33.5, 11.5], [50.5, 7.5, 61.5, 16.5], [-1.5, -2.5, -0.5, 5.5], [3.5, 4.5, 17.5, 15.5], [40.5, -0.5, 47.5, 6.5],
                   [8.5, 1.5, 15.5, 7.5], [-3.5, 6.5, 4.5, 14.5]], F)


def half_product_coords(scale, cells):
    """float32 coordinates x whose float32 product with `scale` is exactly k + 0.5 while the real product lies below it: the fp32 rounding
    of the product moves the cell from k to k + 1 (to -k - 1 for -x)."""
    xs = []
    for k in cells:
        x = F((k + 0.5) / float(F(scale)))
        for _ in range(4):
            if F(x * F(scale)) == F(k + 0.5) and float(x) * float(F(scale)) < k + 0.5:
                xs.append(x)
                break
            x = np.nextafter(x, F(0))
    return xs


def _geo(kind, C):
    H, W = GEO_HW
    rng = np.random.RandomState(100 + C)
    scale = 1.0
    if kind == "halves":
        rois = HALVES
    elif kind == "scale16":                              # the same cells from image coordinates 8, 24, 40, ...
        rois, scale = HALVES * F(16), 0.0625
    elif kind == "scale0.3":
        scale = 0.3                                      # not dyadic: the products are rounded in fp32
        xs = half_product_coords(scale, range(1, 14))
        assert len(xs) >= 4
        rois = [[xs[0], xs[1], xs[-1], xs[-2]], [-xs[0], -xs[1], xs[-3], xs[-1]], [xs[2], xs[0], 150.0, 45.0], [5.0, 15.0, 100.0, 40.0],
                [-4.9, 3.3, 77.7, 51.1], [33.3, 8.4, 199.9, 49.9], [8.333333, 1.666667, 41.666668, 25.0]]
    elif kind == "sides":                                # every side pair 1 .. 14 at one position
        rois = [[3, 1, 3 + rw - 1, 1 + rh - 1] for rh in range(1, 15) for rw in range(1, 15)]
    elif kind == "artefact57":                           # rw = 57: the last bin ends at start + 58
        rois = [[1, 2, 57, 12], [2, 0, 58, 15], [0, 3, 56, 9]]
    elif kind == "artefact114":
        H, W = 3, 120
        rois = [[2, 0, 115, 2], [5, 0, 118, 1], [1, 1, 57, 2], [60, 0, 116, 2]]
    elif kind == "kinds":
        rois = [[30, 10, 20, 4], [10, 12, 40, 3], [25, 5, 18, 11],                                     # inverted
                [-5, 3, 8, 12], [52, 3, 66, 12], [10, -6, 25, 8], [10, 9, 25, 22],                      # partly outside
                [-20, 2, -8, 10], [70, 2, 85, 10], [5, -20, 20, -9], [5, 25, 20, 40],                   # wholly outside
                [-100, -100, 300, 200],                                                                 # far larger than the map
                [0, 0, 0, 0], [W - 1, 0, W - 1, 0], [0, H - 1, 0, H - 1], [W - 1, H - 1, W - 1, H - 1], [W, H, W, H]]
    else:
        raise KeyError(kind)
    feat = distinct_planes(rng, C, H, W)
    if kind.startswith("artefact"):                      # the largest values of every channel in the cell past the box: rw of RoI 0 + its start
        sw, _, ew, _ = roi_cells(np.asarray(rois[0], F), 1.0)
        feat[:, :, ew + 1] += F(2 * H * W)
    return Case("geo:%s/C%d" % (kind, C), feat, np.asarray(rois, F), scale, kind=kind)


GEO_KINDS = ("halves", "scale16", "scale0.3", "sides", "artefact57", "artefact114", "kinds")


def _values(C):
    """NaN, +-inf, plateaus and signed zeros on the 16 x 60 plane; the RoIs sit on the regions."""
    H, W = GEO_HW
    rng = np.random.RandomState(200 + C)
    f = rng.randn(C, H, W).astype(F)
    f[:, 0:9, 0:9] = np.nan                                                  # windows that are all NaN
    f[:, 0:9, 20:29] = -np.inf                                               # ... all -inf
    f[:, 0:9, 10:19] = -FLT_MAX                                              # ... all -FLT_MAX: nothing is above the start value
    m = rng.rand(C, H, 16) < 0.3
    f[:, :, 30:46][m] = np.nan                                               # NaNs inside windows
    f[:, 5, 50] = np.inf
    f[:, 12, 33] = np.inf
    f[:, 14, 38] = -np.inf
    f[:, :, 46:60] = rng.randint(1, 3, (C, H, 14)).astype(F)                 # a plateau of 1s and 2s
    f[:, 5, 50] = np.inf
    z = np.where(rng.rand(C, 7, 20) < 0.5, F(0.0), F(-0.0)).astype(F)
    f[:, 9:16, 0:20] = z                                                     # 0.0 beside -0.0
    rois = [[0, 0, 6, 6], [0, 0, 8, 8], [0, 0, 13, 13], [20, 0, 26, 6], [20, 0, 28, 8], [18, 0, 31, 10], [10, 0, 16, 6], [10, 0, 18, 8],
            [30, 2, 44, 14], [30, 0, 45, 15], [31, 3, 37, 9], [46, 0, 59, 15], [47, 1, 55, 9], [46, 2, 52, 8], [44, 0, 59, 15],
            [0, 9, 19, 15], [2, 10, 12, 15], [0, 9, 6, 15], [0, 0, 59, 15], [3, 3, 5, 5], [32, 11, 34, 13], [-3, -3, 62, 18]]
    return Case("values:/C%d" % C, f, np.asarray(rois, F), 1.0)


LAUNCH_CR = ((4, 1), (4, 257), (512, 40), (512, 42), (512, 84), (512, 512), (1024, 256), (1024, 257), (1028, 3), (5, 300),
             (1, 9), (2, 9), (3, 9), (6, 9), (7, 9))
# (S, RB, exclusive) by the launcher's formulas: S0 = ceil(256 / ceil(C / 4)), S = min(max(S0, ceil(R / 256)), R), RB = ceil(R / S), S = ceil(R / RB);
# exclusive while ceil(C / 4) * S <= 256
LAUNCH_GEOMETRY = {(4, 1): (1, 1, True), (4, 257): (129, 2, True), (512, 40): (2, 20, True), (512, 42): (2, 21, True), (512, 84): (2, 42, True),
                   (512, 512): (2, 256, True), (1024, 256): (1, 256, True), (1024, 257): (2, 129, False), (1028, 3): (1, 3, False),
                   (5, 300): (100, 3, True), (1, 9): (9, 1, True), (2, 9): (9, 1, True), (3, 9): (9, 1, True), (6, 9): (9, 1, True), (7, 9): (9, 1, True)}


def _launch(C, R):
    """5 x 7 planes, distinct values per channel, boxes in and around the map"""
    rng = np.random.RandomState(300 + C + R)
    xy = rng.rand(R, 2) * np.array([9.0, 7.0]) - 2.0
    wh = rng.rand(R, 2) * np.array([9.0, 7.0])
    rois = np.concatenate([xy, xy + wh], 1).astype(F)
    rois[0] = [0, 0, 6, 4]
    return Case("launch:C%d/R%d" % (C, R), distinct_planes(rng, C, 5, 7), rois, 1.0)


STAGING_SHAPES = ((1, 1), (31, 33), (32, 32), (25, 41), (23, 89), (32, 64), (3, 683), (37, 83), (48, 64))           # H*W = 1, 1023 .. 3072
LIMIT_SHAPE = (7, 439)                                                                                               # 3073: one past the LDS forward
BWD16_SHAPES = {(32, 79): "private8", (3, 843): "private4", (48, 64): "private4", (48, 106): "private4", (7, 727): "shared_cb",
                (64, 128): "shared_cb", (3, 2731): None}
BWD32_SHAPES = {(64, 128): "shared_cb", (3, 2731): "one_channel", (128, 128): "one_channel", (5, 3277): "global_atomic"}
BWD_LDS = {("a16", (32, 79)): 163840, ("a16", (48, 106)): 163840, ("a16", (64, 128)): 65536, ("i32", (64, 128)): 65536, ("i32", (128, 128)): 65536}
PLANE_SHAPES = tuple(dict.fromkeys(STAGING_SHAPES + (LIMIT_SHAPE,) + tuple(BWD16_SHAPES) + tuple(BWD32_SHAPES)))


def _plane(H, W, C=2):
    rng = np.random.RandomState(400 + H * 7 + W)
    rois = [[0, 0, W - 1, H - 1], [0, 0, W, H], [-3, -2, W * 0.6, H * 0.7], [W * 0.3, H * 0.2, W + 4, H + 3], [W * 0.4, H * 0.4, W * 0.4 + 2, H * 0.4 + 1],
            [W * 0.1, 0, W * 0.1 + 12, min(H - 1, 11)], [W * 0.5, H * 0.3, W * 0.9, H * 0.95]]
    return Case("plane:%dx%d" % (H, W), distinct_planes(rng, C, H, W), np.asarray(rois, F), 1.0)


RANK_R = 129                         # the recipe draws 129 RoIs; a case takes the first R of them
RANK_CENSUS_R = 64


def _rank(C, H, W, R):
    """A random permutation per channel (all values distinct); sides 7 .. 13 (every fourth RoI, at random: 1 .. 6 on one or both sides) from
    2 cells outside the map to 2 cells outside on the other side."""
    rng = np.random.RandomState(500 + C + H * W)
    feat = distinct_planes(rng, C, H, W)
    rw, rh = rng.randint(7, 14, RANK_R), rng.randint(7, 14, RANK_R)
    small = rng.rand(RANK_R) < 0.25
    small[:2] = False
    which = rng.randint(0, 3, RANK_R)                                        # 0: narrow, 1: low, 2: both
    sm_w, sm_h = rng.randint(1, 7, RANK_R), rng.randint(1, 7, RANK_R)
    rw = np.where(small & (which != 1), sm_w, rw)
    rh = np.where(small & (which != 0), sm_h, rh)
    x0 = np.array([rng.randint(-2, W + 2 - w + 1) for w in rw])             # start -2 .. end W + 1
    y0 = np.array([rng.randint(-2, H + 2 - h + 1) for h in rh])
    x0[0], y0[0] = -2, -2                                                    # (RoIs 0 and 1 of at least 7 x 7 cells, in opposite corners)
    x0[1], y0[1] = W + 2 - rw[1], H + 2 - rh[1]
    rois = np.stack([x0, y0, x0 + rw - 1, y0 + rh - 1], 1).astype(F)
    return Case("rank:C%d/%dx%d/R%d" % (C, H, W, R), feat, rois[:R], 1.0, big=((rw >= 7) & (rh >= 7))[:R])


RANK_NW8_HW, RANK_NW4_HW = (24, 24), (24, 106)                               # 576 pixels: eight copies; 2544 > 2528: four
RANK_CASES = [(C, RANK_NW8_HW, R) for C in (2, 6) for R in (1, 3, 64, 127, 128, 129)] + [(C, RANK_NW4_HW, R) for C in (2, 6) for R in (63, 64, 65)]


@functools.lru_cache(maxsize=None)
def case(name):
    fam, _, rest = name.partition(":")
    if fam == "geo":
        kind, _, c = rest.rpartition("/C")
        return _geo(kind, int(c))
    if fam == "values":
        return _values(int(rest.rpartition("/C")[2]))
    if fam == "launch":
        c, r = rest.split("/")
        return _launch(int(c[1:]), int(r[1:]))
    if fam == "plane":
        h, w = rest.split("x")
        return _plane(int(h), int(w))
    if fam == "rank":
        c, hw, r = rest.split("/")
        h, w = hw.split("x")
        return _rank(int(c[1:]), int(h), int(w), int(r[1:]))
    raise KeyError(name)


GEO_CASES = ["geo:%s/C%d" % (k, c) for k in GEO_KINDS for c in (2, 3)]
VALUE_CASES = ["values:/C2", "values:/C3"]
LAUNCH_CASES = ["launch:C%d/R%d" % cr for cr in LAUNCH_CR]
PLANE_CASES = ["plane:%dx%d" % hw for hw in PLANE_SHAPES]
RANK_NAMES = ["rank:C%d/%dx%d/R%d" % (c, hw[0], hw[1], r) for c, hw, r in RANK_CASES]
ALL_CASES = GEO_CASES + VALUE_CASES + LAUNCH_CASES + PLANE_CASES + RANK_NAMES


@functools.lru_cache(maxsize=None)
def case_ref(name, P=7):
    """(out, argmax) of the case with P x P bins; cached and handed out read-only"""
    c = case(name)
    out, arg = fwd(c.feat, c.rois, P, P, c.scale)
    out.setflags(write=False)
    arg.setflags(write=False)
    return out, arg


@functools.lru_cache(maxsize=None)
def case_bwd(name, P=7):
    """(grad64, n, mag) of the case's integer dOut through the reference's argmax; asserts the exact regime"""
    c = case(name)
    g, n, mag = bwd64(c.go(P, P), case_ref(name, P)[1], c.C, c.H, c.W)
    assert mag.max() < 2 ** 24                                               # every partial sum of every order is an fp32 number
    for a in (g, n, mag):
        a.setflags(write=False)
    return g, n, mag


# ---------------------------------------------------------------------------------------------- censuses (from the reference alone)
def geometry_census(name, P=7):
    """empty bins, raw windows past each of the four sides, and whether another rounding / a float64 product changes the expected output"""
    c = case(name)
    out = {"empty": 0, "left": 0, "right": 0, "top": 0, "bottom": 0}
    for r in range(c.R):
        hs, he, ws, we, raw = roi_windows(c.rois[r], c.scale, P, P, c.H, c.W)
        out["empty"] += int(((he <= hs)[:, None] | (we <= ws)[None, :]).sum())
        out["top"] += int((raw[0] < 0).sum())
        out["bottom"] += int((raw[1] > c.H).sum())
        out["left"] += int((raw[2] < 0).sum())
        out["right"] += int((raw[3] > c.W).sum())
    ref = case_ref(name, P)
    for key, kw in (("half_even_differs", dict(rounding=round_half_even)), ("floor_half_differs", dict(rounding=round_floor_half)),
                    ("f64_product_differs", dict(product=np.float64))):
        alt = fwd(c.feat, c.rois, P, P, c.scale, **kw)
        out[key] = not (np.array_equal(alt[1], ref[1]) and np.array_equal(alt[0].view(np.uint32), ref[0].view(np.uint32)))
    return out


def artefact_census(name):
    """bins of RoI 0 (7 x 7) whose winner lies in the column one past the box's last cell"""
    c = case(name)
    _, _, ew, _ = roi_cells(c.rois[0], c.scale)
    arg = case_ref(name)[1][0]
    return int(((arg >= 0) & (arg % c.W == ew + 1)).sum())


def values_census(name, P=7):
    c = case(name)
    out, arg = case_ref(name, P)
    n = {"all_nan": 0, "all_neginf": 0, "all_fltmin": 0, "nan_skipped": 0, "posinf": int(np.isposinf(out).sum()), "plateau_first": 0,
         "neg_zero": int((out.view(np.uint32) == 0x80000000).sum()), "pos_zero_won": 0, "nan_out": int(np.isnan(out).sum())}
    for r in range(c.R):
        hs, he, ws, we, _ = roi_windows(c.rois[r], c.scale, P, P, c.H, c.W)
        for ph in range(P):
            for pw in range(P):
                if he[ph] <= hs[ph] or we[pw] <= ws[pw]:
                    continue
                for ch in range(c.C):
                    win = c.feat[ch, hs[ph]:he[ph], ws[pw]:we[pw]].reshape(-1)
                    o, a = out[r, ch, ph, pw], arg[r, ch, ph, pw]
                    if np.isnan(win).all():
                        n["all_nan"] += int(o == -FLT_MAX and a == -1)
                    elif np.isneginf(win).all():
                        n["all_neginf"] += int(o == -FLT_MAX and a == -1)
                    elif (win == -FLT_MAX).all():
                        n["all_fltmin"] += int(o == -FLT_MAX and a == -1)
                    elif np.isnan(win).any():
                        n["nan_skipped"] += int(a >= 0 and o == np.nanmax(win))
                    if a >= 0 and (win == o).sum() > 1:
                        ww = int(we[pw] - ws[pw])
                        first = int(np.nonzero(win == o)[0][0])
                        n["plateau_first"] += int(a == (hs[ph] + first // ww) * c.W + ws[pw] + first % ww)
                        n["pos_zero_won"] += int(o == 0 and not np.signbit(o) and np.signbit(win).any())
    return n


SHAPES = {frozenset({(0, 0), (0, 1)}): "pair_h", frozenset({(0, 0), (1, 0)}): "pair_v", frozenset({(0, 0), (1, 1)}): "diag", frozenset({(0, 1), (1, 0)}): "anti",
          frozenset({(0, 0), (0, 1), (1, 0)}): "L_no_br", frozenset({(0, 0), (0, 1), (1, 1)}): "L_no_bl", frozenset({(0, 0), (1, 0), (1, 1)}): "L_no_tr",
          frozenset({(0, 1), (1, 0), (1, 1)}): "L_no_tl", frozenset({(0, 0), (0, 1), (1, 0), (1, 1)}): "full"}


def rank_census(name):
    """Among the bins of the RoIs of at least 7 x 7 cells that share their maximum inside a (RoI, channel): how often each of the nine
    shapes occurs, and for each bin position [channel of the pair, ph, pw] how many sharing groups it belongs to.  A group that is not
    one of the nine shapes (it cannot exist: bins two apart do not overlap) is counted under 'other'."""
    c = case(name)
    arg = case_ref(name)[1]
    shapes = dict.fromkeys(list(SHAPES.values()) + ["other"], 0)
    pos = np.zeros((2, 7, 7), np.int64)
    for r in np.nonzero(c.notes["big"])[0]:
        for ch in range(c.C):
            a = arg[r, ch].reshape(-1)
            for pix in np.unique(a[a >= 0]):
                idx = np.nonzero(a == pix)[0]
                if len(idx) < 2:
                    continue
                ph, pw = idx // 7, idx % 7
                shapes[SHAPES.get(frozenset(zip((ph - ph.min()).tolist(), (pw - pw.min()).tolist())), "other")] += 1
                pos[ch & 1, ph, pw] += 1
    return shapes, pos
