"""A float64 reference of RoIAlign (forward and backward), the generator of the EXACT regime, and the seam cases that
tests/test_roi_align_ref_host.py proves on the CPU and tests/test_gpu_roi_align_exact.py runs against the HIP kernels.

Nothing here is fitted to kernel output.  RoIAlign is bilinear and separable: with Wy[H, PH] (Wx[W, PW]) = the sum over a bin's samples of
the two linear weights a sample puts on its rows (columns),
    backward  dF[c]         = sum over RoIs of  Wy . (dOut[r, c] / cnt) . Wx^T
    forward   out[r, c]     = Wy^T . F[c] . Wx / cnt.
The sample POSITIONS are computed in float32 in the kernels' operation order (b * scale - off, the differences, / PH,
s + bin * b + (i + 0.5) * b / grid; every step rounded, nothing contracted): a float64 position would move a weight by ~2^-24 |position|,
which is not relative to the weight.  Everything after the position is float64.

The exact regime: RoI sides PH * 2^j pixels on a dyadic corner grid, level scales 2^-s, integer dOut.  Every position, weight and product is
then a multiple of a power of two (`unit`), and as long as  max(absgrad) / unit < 2^24  every partial sum of every summation order is an
fp32 number: the kernels must return float32(ref64) in every bit, whatever their tiling, segmenting or atomics do.
"""
import functools

import numpy as np

from oracle import oracle as orc

F = np.float32
PYR_SHAPES = ((100, 168), (50, 84), (25, 42), (13, 21))          # a 672 x 400 frame
PYR_SCALES = (0.25, 0.125, 0.0625, 0.03125)
IMG_WH = (672, 400)


# ---------------------------------------------------------------------------------------------- geometry + weights
def roi_geom(roi, scale, PH, PW, SR, aligned):
    """(sh, sw, bh, bw, gh, gw, cnt): align_geom's numbers, float32 step by step."""
    roi = np.asarray(roi, F)
    s, off = F(scale), F(0.5 if aligned else 0.0)
    sw, sh = F(roi[0] * s) - off, F(roi[1] * s) - off
    ew, eh = F(roi[2] * s) - off, F(roi[3] * s) - off
    rw, rh = F(ew - sw), F(eh - sh)
    if not aligned:
        rw, rh = max(rw, F(1.0)), max(rh, F(1.0))
    bh, bw = F(rh / F(PH)), F(rw / F(PW))
    gh = SR if SR > 0 else int(np.ceil(F(rh / F(PH))))
    gw = SR if SR > 0 else int(np.ceil(F(rw / F(PW))))
    for v in (sh, sw, bh, bw):
        assert type(v) is F or v.dtype == F
    return sh, sw, bh, bw, gh, gw, float(max(gh * gw, 1))


def sample_positions(s0, b, P, G):
    """[P, G] float32: s0 + bin * b + (i + 0.5) * b / G in that order."""
    p = np.arange(P, dtype=F)[:, None]
    i = np.arange(G, dtype=F)[None, :]
    v = (s0 + p * b) + ((i + F(0.5)) * b) / F(G)
    assert v.dtype == F
    return v


def lin_taps(D, v):
    """bilin_setup's rules for one axis: (ok, lo, hi, l) with l = v - lo in float64."""
    ok = ~((v < F(-1.0)) | (v > F(D)))
    v = np.where(v <= 0, F(0.0), v)
    lo = np.minimum(v, F(2 ** 30)).astype(np.int64)
    edge = lo >= D - 1
    lo = np.where(edge, D - 1, lo)
    hi = np.where(edge, D - 1, lo + 1)
    l = np.where(edge, 0.0, v.astype(np.float64) - lo)
    return ok, lo, hi, l


def axis_weights(D, s0, b, P, G):
    """W[D, P] float64: what the G samples of each of the P bins put on each of the D pixels (not yet divided by the sample count)."""
    W = np.zeros((D, P), np.float64)
    if G <= 0:
        return W
    ok, lo, hi, l = lin_taps(D, sample_positions(s0, b, P, G))
    pidx = np.broadcast_to(np.arange(P)[:, None], ok.shape)
    np.add.at(W, (lo[ok], pidx[ok]), (1.0 - l)[ok])
    np.add.at(W, (hi[ok], pidx[ok]), l[ok])
    return W


def roi_weights(roi, H, W, scale, aligned, PH=7, PW=7, SR=2):
    sh, sw, bh, bw, gh, gw, cnt = roi_geom(roi, scale, PH, PW, SR, aligned)
    return axis_weights(H, sh, bh, PH, gh), axis_weights(W, sw, bw, PW, gw), cnt


def _span(Wa):
    nz = np.flatnonzero(np.any(Wa != 0.0, axis=1))
    return (int(nz[0]), int(nz[-1]) + 1) if len(nz) else None


def ref64(go, shape, rois, scale, aligned, level=None, sel=0, PH=7, SR=2):
    """(grad, absgrad) float64 [C, H, W]: the gradient, and the same sum with |go| (every term's magnitude: the scale of any rounding)."""
    C, H, W = shape
    go = np.asarray(go, np.float64)
    rois = np.asarray(rois, F).reshape(-1, 4)
    grad, ab = np.zeros((C, H, W)), np.zeros((C, H, W))
    for r in range(len(rois)):
        if level is not None and level[r] != sel:
            continue
        Wy, Wx, cnt = roi_weights(rois[r], H, W, scale, aligned, PH, PH, SR)
        ys, xs = _span(Wy), _span(Wx)
        if ys is None or xs is None:
            continue
        wy, wxt = Wy[ys[0]:ys[1]], Wx[xs[0]:xs[1]].T
        g = go[r] / cnt
        grad[:, ys[0]:ys[1], xs[0]:xs[1]] += np.matmul(np.matmul(wy, g), wxt)
        ab[:, ys[0]:ys[1], xs[0]:xs[1]] += np.matmul(np.matmul(wy, np.abs(g)), wxt)
    return grad + 0.0, ab          # + 0.0: no negative zeros (the kernels start every sum from +0)


def fwd64(feat, rois, scale, aligned, level=None, sel=0, PH=7, SR=2):
    """out float64 [R, C, PH, PH] from the same Wy / Wx (rows of RoIs on another level stay zero, as the oracle leaves them)."""
    feat = np.asarray(feat, np.float64)
    C, H, W = feat.shape
    rois = np.asarray(rois, F).reshape(-1, 4)
    out = np.zeros((len(rois), C, PH, PH))
    for r in range(len(rois)):
        if level is not None and level[r] != sel:
            continue
        Wy, Wx, cnt = roi_weights(rois[r], H, W, scale, aligned, PH, PH, SR)
        out[r] = np.matmul(np.matmul(Wy.T, feat), Wx) / cnt
    return out + 0.0


def bound_units(n_l):
    """The per-pixel bound of the general-data tests in units of 2^-24 * absgrad, n_l = RoIs mapped to the level.

    Every term of a pixel's sum is dOut * wy * wx / 4, and absgrad is the sum of the terms' magnitudes.  Per TERM, relative to the term:
      2   the two weight roundings (1 - l in each axis; l = v - lo is exact: v and lo lie within a factor of two or lo = 0)
      1   the addition of a bin's two samples into Wx resp. Wy (the 0.25 and the bin's second axis add nothing new: powers of two / same count)
      7   at most 7 FMAs of the column reduction  T[bin row] = sum over bins of dOut * Wx       (one rounding each)
      7   at most 7 FMAs of the row reduction     acc += Wy * T
      31  at most 31 additions of partial tiles (RS_NSEG = 32 segments)
    = 48 roundings of 2^-24 relative each that are NOT additions along the tile's list; the additions along the list (one RoI after the
    other into acc) are at most n_l - 1, each rounding a partial sum that absgrad bounds.  First order in 2^-24: (n_l + 48) * 2^-24 * absgrad."""
    return n_l + 48


# ---------------------------------------------------------------------------------------------- the kernel's tiling, modelled for the premises
RT_TH, RT_TW, RS_SPLIT, RS_NSEG, RS_CHUNK, RA_MAXT, RT_CB = 16, 8, 32, 32, 64, 16, 32


def footprint(roi, H, W, scale, aligned):
    """(y0, y1, x0, x1) inclusive: the pixel box between the first and the last sample of a 7 x 7 / 2 RoI AFTER clamping, whether or not the
    samples count -- a RoI wholly outside the level therefore still 'meets' the border tiles (with all-zero weights), as in the lists kernel."""
    sh, sw, bh, bw, _, _, _ = roi_geom(roi, scale, 7, 7, 2, aligned)
    out = []
    for D, s0, b in ((H, sh, bh), (W, sw, bw)):
        v = sample_positions(s0, b, 7, 2)
        _, lo, hi, _ = lin_taps(D, v)
        out += [int(min(lo[0, 0], lo[6, 1])), int(max(hi[0, 0], hi[6, 1]))]
    return tuple(out)


def tile_lists(rois, shapes, scales, aligned, level):
    """Per level: (counts [tiles_y, tiles_x] of RoIs whose footprint meets the tile, tiles spanned per RoI of the level {r: n})."""
    res = []
    for l, ((H, W), s) in enumerate(zip(shapes, scales)):
        ty, tx = -(-H // RT_TH), -(-W // RT_TW)
        cnt, span = np.zeros((ty, tx), np.int64), {}
        for r in range(len(rois)):
            if level[r] != l:
                continue
            y0, y1, x0, x1 = footprint(rois[r], H, W, s, aligned)
            cnt[y0 // RT_TH:y1 // RT_TH + 1, x0 // RT_TW:x1 // RT_TW + 1] += 1
            span[r] = (y1 // RT_TH - y0 // RT_TH + 1) * (x1 // RT_TW - x0 // RT_TW + 1)
        res.append((cnt, span))
    return res


def nseg(n, split):
    return 0 if n == 0 else 1 if n <= split else min(RS_NSEG, -(-n // split))


def plan(counts, R):
    """The plan of the last lists workgroup: (split threshold, items, cap_items, segment lengths per tile) for the list lengths `counts`."""
    counts = [int(c) for c in counts]
    cap_items = len(counts) + 15 * R // RS_SPLIT + 1
    split = RS_SPLIT
    while sum(nseg(n, split) for n in counts) > cap_items:
        split *= 2
    segs = []
    for n in counts:
        ns = nseg(n, split)
        segs.append([n * (s + 1) // ns - n * s // ns for s in range(ns)])
    return split, sum(len(s) for s in segs), cap_items, segs


# ---------------------------------------------------------------------------------------------- the exact regime
def _pow2(x):
    m, _ = np.frexp(x)
    return bool(np.all(m == 0.5))


def dyadic_unit(rois, level, scales, grid_px, aligned, PH=7, SR=2):
    """The power of two of which every term dOut * wy * wx / cnt (integer dOut) is a multiple, from the RoIs themselves (asserts the regime)."""
    unit = 1.0
    for r, b in enumerate(np.asarray(rois, np.float64)):
        s = float(scales[level[r]])
        assert _pow2(s) and all(float(c) == np.round(c / grid_px) * grid_px for c in b), "corner off the grid"
        u2, g2 = 1.0, 1.0
        for side in (b[2] - b[0], b[3] - b[1]):
            bn = side * s / PH
            assert _pow2(bn) and bn >= 0.25, "bin size %r is no power of two >= 1/4 pixel of the level" % bn
            G = SR if SR > 0 else int(np.ceil(bn))
            assert G & (G - 1) == 0
            u = min(1.0, bn / (2 * G), grid_px * s, 0.5 if aligned else 1.0)
            u2, g2 = u2 * u, g2 * G
        unit = min(unit, u2 / g2)
    assert _pow2(unit)
    return unit


def dyadic_rois(rng, R, img_wh, j_lo, j_hi, grid_px, scales=PYR_SCALES, aligned=False, k_min=2, PH=7, SR=2, square=False, xfrac=1.0):
    """-> (rois [R, 4] float32, unit, level [R] int32).  Sides PH * 2^j pixels, j in [j_lo, j_hi]; width and height differ by one step of j
    (unless `square`), which keeps log2 sqrt(area) a half-integer away from every level boundary: the level is floor((jw + jh) / 2 - 1) up to
    the clamp (for PH = 7, s0 = 224, k0 = 4: log2(7 * 2^j / 224) = j - 5).  Corners on multiples of grid_px; the first eight RoIs stick out of the frame on each
    side, lie wholly outside (both ways) and end in the last row / column; the others start anywhere from half a side before the frame to its end
    (to xfrac of its width: below 1 that leaves the fine levels' right-hand tiles without any RoI)."""
    assert j_hi > j_lo or square
    Wi, Hi = img_wh
    assert grid_px > 0 and _pow2(float(grid_px)) and Wi % grid_px == 0 and Hi % grid_px == 0
    jw = rng.randint(j_lo, j_hi + 1, R)
    d = rng.choice([-1, 1], R)
    jh = jw + d
    jh = np.where((jh < j_lo) | (jh > j_hi), jw - d, jh)
    if square:
        jh = jw.copy()
    w, h = PH * 2.0 ** jw, PH * 2.0 ** jh
    g = float(grid_px)
    x0 = np.floor(rng.uniform(-0.5 * w, xfrac * Wi, R) / g) * g
    y0 = np.floor(rng.uniform(-0.5 * h, Hi, R) / g) * g
    special = [(-0.5, 0.25), (0.25, -0.5), (None, 0.25), (0.25, None), (-4.0, 0.3), (0.3, 9.0), ("far", 0.2), (0.2, "far")]
    for i, (fx, fy) in enumerate(special[:R]):
        for f, c0, side, D in ((fx, x0, w, Wi), (fy, y0, h, Hi)):
            if f is None:                                  # ends beyond the far edge: its last samples clamp to the last row / column
                c0[i] = np.floor((D - 0.5 * side[i]) / g) * g
            elif f == "far":                               # wholly beyond the far edge
                c0[i] = D + np.ceil(2 * side[i] / g) * g
            elif f < 0:                                    # sticks out before the near edge (-4: wholly outside)
                c0[i] = np.floor(f * side[i] / g) * g
            else:
                c0[i] = np.floor(f * max(D - side[i], 0) / g) * g
    rois = np.stack([x0, y0, x0 + w, y0 + h], 1).astype(F)
    assert np.array_equal(rois.astype(np.float64), np.stack([x0, y0, x0 + w, y0 + h], 1))
    if len(scales) > 1:
        assert PH == 7 and not square
        k_max = k_min + len(scales) - 1
        level = (np.clip(np.floor((jw + jh) / 2.0 - 1.0), k_min, k_max) - k_min).astype(np.int32)
        got = orc.roi_level_map(rois, k_min, k_max)
        assert np.array_equal(got, level), "the level map left the half-integer regime"
    else:
        level = np.zeros(R, np.int32)
    return rois, dyadic_unit(rois, level, scales, grid_px, aligned, PH, SR), level


def int_go(rng, R, C, PH=7, amp=8):
    return rng.randint(-amp, amp + 1, (R, C, PH, PH)).astype(F)


# ---------------------------------------------------------------------------------------------- the cases
class Case(dict):
    __getattr__ = dict.__getitem__


def _case(name, rng, shapes, scales, C, R, j, grid_px=2, aligned=False, amp=8, img_wh=None, PH=7, SR=2, square=False, xfrac=1.0, branch=""):
    if img_wh is None:
        img_wh = (int(round(shapes[0][1] / scales[0])), int(round(shapes[0][0] / scales[0])))
    rois, unit, level = dyadic_rois(rng, R, img_wh, j[0], j[1], grid_px, scales, aligned, 2, PH, SR, square, xfrac)
    return Case(name=name, shapes=tuple(shapes), scales=tuple(scales), C=C, R=R, rois=rois, level=level, unit=unit, aligned=aligned,
                go=int_go(rng, R, C, PH, amp), PH=PH, SR=SR, branch=branch)


ONE_TILE = dict(shapes=((16, 8),), scales=(1.0 / 16,))
SEG_LENGTHS = (1, 32, 33, 64, 65, 1024, 1025, 2080, 2081)
CHUNK_R = (255, 256, 257, 513)
REG_PATH_C = (3, 33, 40)
LEVEL_SHAPES = ((13, 21), (25, 42), (1, 3), (16, 8), (17, 9))
GENERIC = ((4, 2), (7, 4), (8, 0))
RESIDENT_MIN, RESIDENT_MAX = 256 * 5, 256 * 6          # workgroups of the tile kernel the device holds: 256 CUs x occupancy 5 or 6


@functools.lru_cache(maxsize=None)
def case(name):
    """The exact cases by name.  Each is deterministic (its own seed) and small; `branch` says what it reaches."""
    kind, _, arg = name.partition(":")
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31)
    rng = np.random.RandomState(seed)
    if kind == "seg":          # one 16 x 8 level = ONE tile that owns every RoI: list length = R
        n = int(arg)
        long_ = n >= 1024
        return _case(name, rng, C=32, R=n, j=(3, 5) if long_ else (2, 5), amp=2 if long_ else 8, **ONE_TILE,
                     branch="one tile, list of %d: %s" % (n, "unsplit, written straight to the plane" if n <= 32 else "split into segments, last arriver combines"))
    if kind == "chunk":        # the lists kernel scans the RoIs in chunks of 256
        return _case(name, rng, ((50, 84),), (1.0 / 16,), 32, int(arg), (2, 6), branch="lists kernel: %s RoIs = chunks of 256 and a remainder" % arg)
    if kind == "regC":         # C % 32 != 0: the register instantiation, partial last channel group
        return _case(name, rng, ((50, 84),), (1.0 / 16,), int(arg), 150, (2, 6), branch="register path, C = %s" % arg)
    if kind == "dma64":        # also run with grad_out one float into a larger buffer
        return _case(name, rng, ((50, 84),), (1.0 / 16,), 64, 150, (2, 6), branch="LDS-DMA path (aligned) / register path with whole groups (misaligned)")
    if kind == "mixed":        # j = 2..4: at most 3 x 5 tiles (records); j = 6, 7: 28+ level pixels tall AND 56 wide -> more than 16 tiles (tables built in the tile kernel)
        a = _case(name, rng, ((50, 84),), (1.0 / 16,), 64, 160, (2, 4))
        b = _case(name + "b", rng, ((50, 84),), (1.0 / 16,), 64, 160, (6, 7))
        pick = (np.arange(160) % 3 == 2)
        w, h = (b.rois[:, 2] - b.rois[:, 0]).astype(np.float64), (b.rois[:, 3] - b.rois[:, 1]).astype(np.float64)
        x0 = np.floor(rng.uniform(0, 1, 160) * np.maximum(1344 - w, 0) / 2) * 2      # the large ones lie inside the frame as far as they fit
        y0 = np.floor(rng.uniform(0, 1, 160) * np.maximum(800 - h, 0) / 2) * 2
        a["rois"] = np.where(pick[:, None], np.stack([x0, y0, x0 + w, y0 + h], 1), a.rois).astype(F)
        a["unit"] = min(a.unit, b.unit)
        a["branch"] = "records and in-kernel tables interleaved in the same lists"
        return a
    if kind == "coarsen":      # 512 RoIs of 896 x 896 pixels on a 1344 x 800 frame: each covers all rows and two thirds of the columns of the 50 x 84 level
        c = _case(name, rng, ((50, 84),), (1.0 / 16,), 64, 512, (7, 7), amp=2, square=True, branch="plan doubles the split threshold")
        x0 = (rng.randint(0, 225, 512) * 2.0).astype(F)
        y0 = (rng.randint(-24, 1, 512) * 2.0).astype(F)
        c["rois"] = np.stack([x0, y0, x0 + F(896.0), y0 + F(896.0)], 1).astype(F)
        return c
    if kind == "pyr":          # four levels, R = 600: C = 64 keeps cap_items * n_cg below the resident count, C = 128 puts it above
        Cc = int(arg)
        return _case(name, rng, PYR_SHAPES, PYR_SCALES, Cc, 600, (2, 7), img_wh=IMG_WH, xfrac=0.6,
                     branch="four levels; item blocks %s one round of resident workgroups" % ("within" if Cc <= 64 else "exceed"))
    if kind == "pyr_empty":    # j >= 4 on both axes: nothing maps to level 0
        c = _case(name, rng, PYR_SHAPES, PYR_SCALES, 32, 120, (4, 7), img_wh=IMG_WH, branch="level 0 has no RoI: every tile of it is zero-filled")
        assert not (c.level == 0).any() and set(c.level.tolist()) == {1, 2, 3}
        return c
    if kind == "shape":
        H, W = (int(v) for v in arg.split("x"))
        return _case(name, rng, ((H, W),), (1.0 / 16,), 32, 60, (2, 5), img_wh=(W * 16, H * 16), branch="level %s" % arg)
    if kind == "aligned":      # aligned = 1: positions b * scale - 0.5, no clamp of the RoI size
        if arg == "pyr":
            return _case(name, rng, PYR_SHAPES, PYR_SCALES, 32, 200, (2, 7), aligned=True, img_wh=IMG_WH, branch="aligned = 1, four levels")
        return _case(name, rng, ((50, 84),), (1.0 / 16,), 40, 150, (2, 6), aligned=True, branch="aligned = 1, register path")
    if kind == "b2b":          # the sequence of back-to-back calls takes its RoIs from this one
        return _case(name, rng, PYR_SHAPES, PYR_SCALES, 32, 600, (2, 7), img_wh=IMG_WH, branch="back-to-back calls on one workspace")
    if kind == "generic":      # the scatter kernels: memset + fp32 atomics; sample count a power of two
        PH, SR = (int(v) for v in arg.split("/"))
        return _case(name, rng, ((50, 84),), (1.0 / 16,), 8, 80, (4, 6) if SR == 0 else (2, 6), PH=PH, SR=SR, square=(SR == 0),
                     branch="generic kernels, %d x %d bins, sampling ratio %d" % (PH, PH, SR))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_ref(name, R=None):
    """[(grad, absgrad)] per level of case(name) (its first R RoIs), computed once and shared; callers do not modify it."""
    c = case(name)
    n = c.R if R is None else R
    out = [ref64(c.go[:n], (c.C, h, w), c.rois[:n], s, c.aligned, c.level[:n], l, c.PH, c.SR) for l, ((h, w), s) in enumerate(zip(c.shapes, c.scales))]
    for g, a in out:
        g.setflags(write=False)
        a.setflags(write=False)
    return out


def check_premise(name, R=None):
    """The exactness premise of a case: every term is a multiple of `unit` and no sum of magnitudes reaches 2^24 units."""
    c = case(name)
    worst = 0.0
    for g, a in case_ref(name, R):
        assert np.array_equal(np.round(g / c.unit), g / c.unit) and np.array_equal(np.round(a / c.unit), a / c.unit), name
        worst = max(worst, float(a.max()) / c.unit)
    assert worst < 2 ** 24, (name, worst)
    return worst


EXACT_CASES = (["seg:%d" % n for n in SEG_LENGTHS] + ["chunk:%d" % r for r in CHUNK_R] + ["regC:%d" % c for c in REG_PATH_C]
               + ["dma64:", "mixed:", "coarsen:", "pyr:64", "pyr:128", "pyr_empty:"] + ["shape:%dx%d" % s for s in LEVEL_SHAPES]
               + ["aligned:pyr", "aligned:one", "b2b:"] + ["generic:%d/%d" % g for g in GENERIC])


# ---------------------------------------------------------------------------------------------- general data
def general_rois(rng, R, img_wh):
    """Non-dyadic RoIs, log-uniform in size, plus the four edge boxes of the older tests."""
    Wi, Hi = img_wh
    c = rng.uniform(0.05, 0.95, (R, 2))
    wh = np.exp(rng.uniform(np.log(0.02), np.log(0.9), (R, 2)))
    rois = (np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1) * np.array([Wi, Hi, Wi, Hi])).astype(F)
    rois[0] = [-0.045 * Wi, -0.05 * Hi, 0.27 * Wi, 0.37 * Hi]         # partly outside
    rois[1] = [0, 0, Wi, Hi]                                          # the whole frame
    rois[2] = [0.4 * Wi + 0.5, 0.4 * Hi + 0.5, 0.4 * Wi + 0.7, 0.4 * Hi + 0.6]   # tiny: clamped to 1 x 1
    rois[3] = [Wi - 1.5, Hi - 1.5, Wi + 3, Hi + 3]                    # bottom-right corner clamp
    return rois


@functools.lru_cache(maxsize=None)
def general_case(name):
    rng = np.random.RandomState(77 if name == "pyr" else 78)
    if name == "pyr":
        shapes, scales, C, R, img = PYR_SHAPES, PYR_SCALES, 64, 512, IMG_WH
    else:
        shapes, scales, C, R, img = ((50, 84),), (1.0 / 16,), 40, 512, (1344, 800)
    rois = general_rois(rng, R, img)
    level = orc.roi_level_map(rois) if len(shapes) > 1 else np.zeros(R, np.int32)
    return Case(name=name, shapes=shapes, scales=scales, C=C, R=R, rois=rois, level=level, aligned=False, go=rng.randn(R, C, 7, 7).astype(F), PH=7, SR=2)


@functools.lru_cache(maxsize=None)
def general_ref(name):
    c = general_case(name)
    return [ref64(c.go, (c.C, h, w), c.rois, s, False, c.level, l) for l, ((h, w), s) in enumerate(zip(c.shapes, c.scales))]
