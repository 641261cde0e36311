"""An independent restatement of the two target makers (RPNTargetMaker.forward, FastRcnnTargetMaker.forward) on EXACT data, and
the generators of the seam cases that tests/test_targets_ref_host.py (CPU) and tests/test_gpu_targets_exact.py (GPU) run.
Plain Python / numpy: it imports nothing of the project and nothing of the C oracle.

Boxes live on a lattice: a coordinate is an integer k and means k / 32 (k in [0, 32] is the image; RPN fillers may lie outside).
Everything is computed in lattice units with integers and fractions.Fraction:
  inter, union : integers (areas in units of 1/1024)
  IoU          : variant 1 (util/box_ops.py:24-37) the exact rational inter / union;
                 variant 0 (utils/util.py:66-102) inter / (union + eps), eps = the exact value of float32(1e-5) in those units.
An fp32 implementation computes inter and union exactly on this lattice (10-bit coordinates, 20-bit products), so it differs from
the rational only by the rounding of `union + eps` and of the division: at most 2 * 2^-24 relative.  check_decidable() is the
guard that makes this harmless: every comparison a case's result depends on is
  * between identical (inter, union) pairs (an intersection of 0 is the same +0 whatever the union), or
  * variant 1 only, an exact threshold hit: inter / union is exactly 7/10, 3/10 or 1/2, and the fp32 division of the two integers
    gives 0.7f, 0.3f, 0.5f (evaluated here with numpy for the very pair), or
  * separated by a relative margin above 2^-18.
The rules themselves are taken from the reference's text:
  RPN variant 0, models/model_.py:186-266: only anchors inside [0, 1]; label 0 if the row maximum < 0.3 (:202); label 1 for THE
    argmax anchor of every gt, torch's max(dim=0) = the lowest index (:206,:213); label 1 if the row maximum >= 0.7 (:216);
    sampling :225-236; targets encode(gt[argmax], anchor) (:253), zeros and label -1 outside (:256-263).
  RPN variant 1, models/new_model.py:299-349: all anchors; every anchor whose IoU EQUALS a gt's maximum is positive (:316-318).
  Head, models/model_.py:127-179 and models/new_model.py:157-206: candidates [rois; gt]; positive if max >= 0.5, negative if
    0 <= max < 0.5; class gt_label[first argmax] + label_offset; targets encode / (0.1, 0.1, 0.2, 0.2).
Sampling takes the permutations as input (the reference draws them with torch.randperm)."""
import math
from fractions import Fraction

import numpy as np

LAT = 32
EPS32 = Fraction(float(np.float32(1e-5)))            # the exact value of the fp32 constant
EPS_LAT = EPS32 * LAT * LAT                          # in lattice-area units
MARGIN = Fraction(1, 1 << 18)
T03, T05, T07 = Fraction(3, 10), Fraction(1, 2), Fraction(7, 10)
STD = (Fraction(float(np.float32(0.1))), Fraction(float(np.float32(0.1))), Fraction(float(np.float32(0.2))), Fraction(float(np.float32(0.2))))
HT_ERR_SHORT = 8


def to_f32(boxes):
    """lattice integers -> the fp32 boxes the kernels and the oracle see (exact)"""
    return (np.asarray(boxes, np.int64).reshape(-1, 4).astype(np.float64) / LAT).astype(np.float32)


def f32_of(fr):
    """the fp32 rounding (nearest even) of an exact rational, as a Python float; normal range only"""
    if fr == 0:
        return 0.0
    s, fr = (-1.0, -fr) if fr < 0 else (1.0, fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    assert Fraction(2) ** e <= fr < Fraction(2) ** (e + 1) and -120 < e < 120
    q = fr * Fraction(2) ** (23 - e)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    return s * math.ldexp(n, e - 23)


# ------------------------------------------------------------------------------------------------ the exact IoU table
def _keys(c, g):
    """(inter << 32 | union) of every (candidate, gt) pair; an empty intersection is the one key 1"""
    w = np.minimum(c[:, None, 2], g[None, :, 2]) - np.maximum(c[:, None, 0], g[None, :, 0])
    h = np.minimum(c[:, None, 3], g[None, :, 3]) - np.maximum(c[:, None, 1], g[None, :, 1])
    inter = np.clip(w, 0, None) * np.clip(h, 0, None)
    ac = (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])
    ag = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    union = ac[:, None] + ag[None, :] - inter
    assert (union >= 0).all() and (inter < (1 << 30)).all() and (union < (1 << 31)).all()
    return np.where(inter == 0, np.int64(1), (inter << 32) | union), (inter == 0) & (union == 0)


class IouTable:
    """The IoU of every candidate against every gt as exact rationals, held as dense ranks of the distinct values so that maxima,
    first argmaxima and equalities are integer operations.  Walked in row blocks: the largest case has 17 M pairs."""

    def __init__(self, cand, gt, variant):
        self.c = np.asarray(cand, np.int64).reshape(-1, 4)
        self.g = np.asarray(gt, np.int64).reshape(-1, 4)
        self.variant = variant
        self.n, self.G = self.c.shape[0], self.g.shape[0]
        self.step = max(1, (1 << 21) // self.G)
        keys = np.zeros(0, np.int64)
        self.zero_over_zero = False
        for lo in range(0, self.n, self.step):
            k, zz = _keys(self.c[lo:lo + self.step], self.g)
            self.zero_over_zero |= bool(zz.any())
            keys = np.union1d(keys, np.unique(k))
        self.keys = keys
        self.pairs = [(0, 1) if int(k) == 1 else (int(k) >> 32, int(k) & 0xFFFFFFFF) for k in keys]
        vals = [self.value(i, u) for i, u in self.pairs]
        order = sorted(range(len(vals)), key=lambda j: vals[j])
        self.rank_of_uid = np.empty(len(vals), np.int64)
        self.val_of_rank, self.uids_of_rank = [], []
        for j in order:
            if not self.val_of_rank or vals[j] != self.val_of_rank[-1]:
                self.val_of_rank.append(vals[j])
                self.uids_of_rank.append([])
            self.rank_of_uid[j] = len(self.val_of_rank) - 1
            self.uids_of_rank[-1].append(j)
        self._rows()

    def value(self, inter, union):
        if inter == 0:
            return Fraction(0)
        return Fraction(inter, union) if self.variant == 1 else Fraction(inter) / (union + EPS_LAT)

    def block(self, lo):
        uid = np.searchsorted(self.keys, _keys(self.c[lo:lo + self.step], self.g)[0])
        return uid, self.rank_of_uid[uid]

    def _rows(self):
        n, G = self.n, self.G
        self.row_max = np.empty(n, np.int64)          # rank of the row maximum
        self.row_arg = np.empty(n, np.int64)          # its first gt
        self.row_second = np.empty(n, np.int64)       # rank of the largest value below it, -1 if none
        self.row_tie_same = np.empty(n, bool)         # every entry AT the maximum is the same (inter, union) pair
        self.col_max = np.full(G, -1, np.int64)
        self.col_first = np.zeros(G, np.int64)        # lowest candidate index that attains the column maximum
        self.col_second = np.full(G, -1, np.int64)
        cu_lo = np.zeros(G, np.int64)
        cu_hi = np.zeros(G, np.int64)
        for lo in range(0, n, self.step):
            uid, R = self.block(lo)
            m = R.shape[0]
            rm = R.max(1)
            at = R == rm[:, None]
            self.row_max[lo:lo + m] = rm
            self.row_arg[lo:lo + m] = at.argmax(1)
            self.row_second[lo:lo + m] = np.where(at, -1, R).max(1)
            self.row_tie_same[lo:lo + m] = np.where(at, uid, 1 << 40).min(1) == np.where(at, uid, -1).max(1)
            cm = R.max(0)
            atc = R == cm[None, :]
            cs = np.where(atc, -1, R).max(0)
            ulo, uhi = np.where(atc, uid, 1 << 40).min(0), np.where(atc, uid, -1).max(0)
            first = atc.argmax(0) + lo
            new = cm > self.col_max
            same = cm == self.col_max
            second = np.maximum(np.where(new, np.maximum(self.col_max, cs), np.where(same, np.maximum(self.col_second, cs),
                                                                                     np.maximum(self.col_second, cm))), -1)
            self.col_first = np.where(new, first, self.col_first)
            cu_lo = np.where(new, ulo, np.where(same, np.minimum(cu_lo, ulo), cu_lo))
            cu_hi = np.where(new, uhi, np.where(same, np.maximum(cu_hi, uhi), cu_hi))
            self.col_second = second
            self.col_max = np.maximum(self.col_max, cm)
        self.col_tie_same = cu_lo == cu_hi

    def equals_a_col_max(self):
        """[n] bool: the candidate's IoU with some gt equals that gt's maximum; and [G] how many candidates attain each maximum"""
        out = np.zeros(self.n, bool)
        cnt = np.zeros(self.G, np.int64)
        for lo in range(0, self.n, self.step):
            _, R = self.block(lo)
            eq = R == self.col_max[None, :]
            out[lo:lo + R.shape[0]] = eq.any(1)
            cnt += eq.sum(0)
        return out, cnt

    def row_value(self, i):
        return self.val_of_rank[self.row_max[i]]

    # ---- the guard's pieces
    def _separated(self, hi_rank, lo_rank):
        a, b = self.val_of_rank[hi_rank], self.val_of_rank[lo_rank]
        return a > b and (a - b) > MARGIN * a

    def _threshold_ok(self, rank, t):
        """the value of `rank` against threshold t: an exact hit fp32 reproduces (variant 1), or a clear margin"""
        v = self.val_of_rank[rank]
        if v == t:
            if self.variant != 1:
                return False
            return all(np.float32(i) / np.float32(u) == np.float32(float(t)) for i, u in (self.pairs[j] for j in self.uids_of_rank[rank]))
        return abs(v - t) > MARGIN * t

    def undecidable(self, thresholds, columns):
        """the list of reasons why fp32 might decide a comparison of this table differently (empty = decidable)"""
        bad = []
        if self.zero_over_zero and self.variant == 1:
            bad.append("0/0 in variant 1")
        if not self.row_tie_same.all():
            bad.append("row %d: its maximum is shared by different (inter, union) pairs" % int(np.nonzero(~self.row_tie_same)[0][0]))
        for hi, lo in {(int(a), int(b)) for a, b in zip(self.row_max, self.row_second) if b >= 0}:
            if not self._separated(hi, lo):
                bad.append("row maximum %s too close to %s" % (self.val_of_rank[hi], self.val_of_rank[lo]))
        for r in {int(a) for a in self.row_max}:
            for t in thresholds:
                if not self._threshold_ok(r, t):
                    bad.append("row maximum %s undecidable against %s" % (self.val_of_rank[r], t))
        if columns:
            if not self.col_tie_same.all():
                bad.append("gt %d: its maximum is shared by different (inter, union) pairs" % int(np.nonzero(~self.col_tie_same)[0][0]))
            for hi, lo in {(int(a), int(b)) for a, b in zip(self.col_max, self.col_second) if b >= 0}:
                if not self._separated(hi, lo):
                    bad.append("column maximum %s too close to %s" % (self.val_of_rank[hi], self.val_of_rank[lo]))
        return bad


# ------------------------------------------------------------------------------------------------ encode
def _div(num, den):
    """IEEE semantics for a zero divisor; otherwise the exact rational"""
    if den == 0:
        return float("nan") if num == 0 else math.copysign(float("inf"), num)
    return Fraction(num) / den


def encode_exact(g, a):
    """encode(xy_to_cxcy(g), xy_to_cxcy(a)) of lattice boxes (utils/util.py:39-43): columns 0-1 exact (Fraction, or +-inf / nan for a
    zero divisor), columns 2-3 as float64 log."""
    g = [int(v) for v in g]
    a = [int(v) for v in a]
    gw, gh, aw, ah = g[2] - g[0], g[3] - g[1], a[2] - a[0], a[3] - a[1]
    dx = _div(Fraction(g[2] + g[0] - a[2] - a[0], 2), aw)
    dy = _div(Fraction(g[3] + g[1] - a[3] - a[1], 2), ah)

    def lg(p, q):
        if q == 0:
            return float("nan") if p == 0 else float("inf")
        return float("-inf") if p == 0 else math.log(p / q)
    return dx, dy, lg(gw, aw), lg(gh, ah)


def _f32_or_special(v):
    return v if isinstance(v, float) else f32_of(v)


# ------------------------------------------------------------------------------------------------ RPN
class RpnCase:
    def __init__(self, name, variant, anchors, gt, seam):
        self.name, self.variant = name, variant
        self.anchors = np.asarray(anchors, np.int64).reshape(-1, 4)
        self.gt = np.asarray(gt, np.int64).reshape(-1, 4)
        self.seam = seam                              # callable(case, result) -> None, asserts that the case holds what it is named for
        self._res = None

    @property
    def N(self):
        return self.anchors.shape[0]

    @property
    def G(self):
        return self.gt.shape[0]


class RpnResult:
    pass


def rpn_match(case):
    """labels before sampling, first-argmax gt, counts, regression targets (cached on the case)"""
    if case._res is not None:
        return case._res
    a, N = case.anchors, case.N
    if case.variant == 1:
        part = np.ones(N, bool)
    else:
        part = (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] <= LAT) & (a[:, 3] <= LAT)
    idx = np.nonzero(part)[0]
    assert len(idx) > 0, "the reference fails without an anchor inside the image"
    tab = IouTable(a[idx], case.gt, case.variant)
    lab = np.full(len(idx), -1, np.int64)
    rowv = np.array([v < T03 for v in tab.val_of_rank])[tab.row_max]
    lab[rowv] = 0
    eq, cnt = tab.equals_a_col_max()
    if case.variant == 1:
        lab[eq] = 1
    else:
        lab[tab.col_first] = 1
    lab[np.array([v >= T07 for v in tab.val_of_rank])[tab.row_max]] = 1
    r = RpnResult()
    r.part, r.idx, r.tab, r.col_count = part, idx, tab, cnt
    r.pre = np.full(N, -1, np.int64)
    r.pre[idx] = lab
    r.arg = np.zeros(N, np.int64)
    r.arg[idx] = tab.row_arg
    r.col_first = idx[tab.col_first]                  # anchor index of every gt's lowest-index best anchor
    r.n_pos, r.n_neg = int((lab == 1).sum()), int((lab == 0).sum())
    memo = {}
    r.reg01 = np.zeros((N, 2), np.float32)            # the fp32 rounding of the exact rational
    r.reg23 = np.zeros((N, 2), np.float64)
    for i in idx:
        key = (tuple(a[i]), int(r.arg[i]))
        if key not in memo:
            e = encode_exact(case.gt[r.arg[i]], a[i])
            memo[key] = ((_f32_or_special(e[0]), _f32_or_special(e[1])), (e[2], e[3]))
        r.reg01[i], r.reg23[i] = memo[key]
    case._res = r
    return r


def rpn_sample(case, perm_pos=None, perm_neg=None):
    """models/model_.py:225-236: labels after sampling with the given permutations"""
    r = rpn_match(case)
    lab = r.pre.copy()
    n_pos, n_neg = r.n_pos, r.n_neg
    if n_pos > 128 and perm_pos is not None:
        assert len(perm_pos) == n_pos
        lab[np.nonzero(r.pre == 1)[0][np.asarray(perm_pos)[128:]]] = -1
    if n_neg > 256 - n_pos and perm_neg is not None:
        assert len(perm_neg) == n_neg
        lab[np.nonzero(r.pre == 0)[0][np.asarray(perm_neg)[256 - min(n_pos, 128):]]] = -1
    return lab


# ------------------------------------------------------------------------------------------------ head
class HeadCase:
    def __init__(self, name, variant, rois, gt, gt_label, seam, n_rois=None, max_pos=None, total=None):
        self.name, self.variant = name, variant
        self.rois = np.asarray(rois, np.int64).reshape(-1, 4)         # P_cap rows; rows behind n_rois are never read
        self.gt = np.asarray(gt, np.int64).reshape(-1, 4)
        self.gt_label = np.asarray(gt_label, np.int64)
        self.n_rois = self.rois.shape[0] if n_rois is None else n_rois
        self.label_offset = 1 if variant == 0 else 0
        self.max_pos = (32 if variant == 0 else 128) if max_pos is None else max_pos
        self.total = (128 if variant == 0 else 512) if total is None else total
        self.seam = seam
        self._res = None

    @property
    def n(self):
        return self.n_rois + self.gt.shape[0]

    def rois_f32(self):
        """what the device is handed: P_cap rows, NaN behind the live ones"""
        out = to_f32(self.rois)
        out[self.n_rois:] = np.nan
        return out


class HeadResult:
    pass


def head_match(case):
    if case._res is not None:
        return case._res
    r = HeadResult()
    r.cand = np.concatenate([case.rois[:case.n_rois], case.gt])
    r.tab = IouTable(r.cand, case.gt, case.variant)
    pos = np.array([v >= T05 for v in r.tab.val_of_rank])[r.tab.row_max]
    r.pos_list, r.neg_list = np.nonzero(pos)[0], np.nonzero(~pos)[0]         # (a finite maximum is never below 0)
    r.npc, r.nnc = len(r.pos_list), len(r.neg_list)
    r.arg = r.tab.row_arg
    case._res = r
    return r


def head_sample(case, perm_pos, perm_neg):
    """-> keep [rows], cls [rows], reg01 [rows, 2] fp32 exact, reg23 [rows, 2] float64, counts [npc, nnc, rows, err]"""
    r = head_match(case)
    assert len(perm_pos) == r.npc and len(perm_neg) == r.nnc
    n_pos = min(r.npc, case.max_pos)
    n_neg = min(case.total - n_pos, r.nnc)
    keep = np.concatenate([r.pos_list[np.asarray(perm_pos, np.int64)[:n_pos]], r.neg_list[np.asarray(perm_neg, np.int64)[:n_neg]]]).astype(np.int64)
    cls = case.gt_label[r.arg[keep]] + case.label_offset
    cls[n_pos:] = 0
    reg01 = np.zeros((len(keep), 2), np.float32)
    reg23 = np.zeros((len(keep), 2), np.float64)
    for j, k in enumerate(keep):
        e = encode_exact(case.gt[r.arg[k]], r.cand[k])
        reg01[j] = [f32_of(Fraction(f32_of(e[0])) / STD[0]), f32_of(Fraction(f32_of(e[1])) / STD[1])]
        reg23[j] = [e[2] / 0.2, e[3] / 0.2]
    rows = n_pos + n_neg
    return keep, cls, reg01, reg23, [r.npc, r.nnc, rows, HT_ERR_SHORT if rows < case.total else 0]


# ------------------------------------------------------------------------------------------------ the guard
def check_decidable(case):
    """Raises AssertionError with the reasons if an fp32 evaluation could decide any comparison of the case differently."""
    if isinstance(case, RpnCase):
        bad = rpn_match(case).tab.undecidable((T03, T07), columns=True)
    else:
        bad = head_match(case).tab.undecidable((T05,), columns=False)
    assert not bad, "%s is not decidable in fp32: %s" % (case.name, "; ".join(bad[:5]))


# ------------------------------------------------------------------------------------------------ building blocks of the cases
# 256 "slots" (p, q), p, q in [0, 16): a unit-square gt at (2p, 2q) with two different anchors that both contain it and have twice its
# area -- IoU exactly 1/2 = (1, 2) -- and touch no other slot's gt.
def slot_gt(s):
    p, q = s % 16, s // 16
    return [2 * p, 2 * q, 2 * p + 1, 2 * q + 1]


def slot_h(s):
    p, q = s % 16, s // 16
    return [2 * p, 2 * q, 2 * p + 2, 2 * q + 1]


def slot_v(s):
    p, q = s % 16, s // 16
    return [2 * p, 2 * q, 2 * p + 1, 2 * q + 2]


BLANKET = [0, 0, LAT, LAT]
FILL_V0 = [-16, -16, -8, -8]                  # outside the image: label -1, target 0
FILL_V1 = [0, 0, LAT, 2 * LAT]                # IoU exactly 1/2 with the blanket gt: label -1, never a column maximum


def assemble_rpn(name, variant, N, placed, gts, seam):
    """anchors: `placed` {index: box}, fillers elsewhere.  Variant 1 with fillers gets the blanket gt LAST and its exact copy at a free
    index, so the fillers come out -1."""
    placed = dict(placed)
    gts = [list(g) for g in gts]
    if variant == 1 and len(placed) < N:
        gts.append(BLANKET)
        free = next(i for i in list(range(N // 2, N)) + list(range(N // 2)) if i not in placed)
        placed[free] = BLANKET
    fill = FILL_V0 if variant == 0 else FILL_V1
    anchors = np.tile(np.asarray(fill, np.int64), (N, 1))
    for i, b in placed.items():
        assert 0 <= i < N
        anchors[i] = b
    return RpnCase(name, variant, anchors, gts, seam)


def _scatter(rng, N, k, fixed=()):
    """k distinct anchor indices over [0, N): the fixed ones first, the rest drawn"""
    rest = [i for i in rng.permutation(N) if i not in set(fixed)]
    return list(fixed) + [int(i) for i in rest[:k - len(fixed)]]


# ------------------------------------------------------------------------------------------------ RPN cases
def _neg_box(k):
    """a unit square in the region x, y >= 22, which no gt of any case below reaches; 100 different ones"""
    return [22 + k % 10, 22 + (k // 10) % 10, 23 + k % 10, 23 + (k // 10) % 10]


TIE_N = 1500
TIE_PAIRS = [(5, 6), (70, 134), (255, 256), (1023, 1024), (0, TIE_N - 1), (300, 900)]


def rpn_tie_case(variant, swap):
    """slot k's gt has two best anchors at IoU 1/2: H and V boxes (different boxes, the same (inter, union)) at TIE_PAIRS[k]; the last
    pair holds two IDENTICAL boxes.  swap: the other box first."""
    placed = {}
    for k, (i, j) in enumerate(TIE_PAIRS):
        b0, b1 = (slot_h(k), slot_v(k)) if k < len(TIE_PAIRS) - 1 else (slot_h(k), slot_h(k))
        placed[i], placed[j] = (b1, b0) if swap else (b0, b1)

    def seam(c, r):
        for k, (i, j) in enumerate(TIE_PAIRS):
            assert r.col_count[k] == 2 and r.col_first[k] == i, k
            assert r.tab.val_of_rank[r.tab.col_max[k]] == (T05 if variant == 1 else Fraction(1) / (2 + EPS_LAT))
            assert (r.pre[i], r.pre[j]) == ((1, 1) if variant == 1 else (1, -1)), k
            assert k == len(TIE_PAIRS) - 1 or tuple(c.anchors[i]) != tuple(c.anchors[j])
    return assemble_rpn("tie-v%d-%s" % (variant, "swapped" if swap else "straight"), variant, TIE_N, placed, [slot_gt(k) for k in range(len(TIE_PAIRS))], seam)


def rpn_symmetric_tie_case(variant):
    """the issue's own example: [0,0,16,32] and [0,0,32,16] against gt [0,0,16,16]"""
    def seam(c, r):
        assert r.col_count[0] == 2 and r.col_first[0] == 1
        assert r.pre[1] == 1 and r.pre[2] == (1 if variant == 1 else -1)
    return RpnCase("tie-symmetric-v%d" % variant, variant, [[20, 20, 24, 24], [0, 0, 16, 32], [0, 0, 32, 16]], [[0, 0, 16, 16]], seam)


THRESH_ANCHORS = [
    ("copy", [0, 0, 30, 30], 1, 1),
    ("7/10", [0, 0, 30, 21], 1, -1),                 # exactly 7/10: >= 0.7 in variant 1; below it with eps
    ("7/10 - step", [0, 0, 29, 21], -1, -1),
    ("7/10 + step", [0, 0, 30, 22], 1, 1),
    ("3/10", [0, 0, 30, 9], -1, 0),                  # exactly 3/10: not < 0.3 in variant 1; below it with eps
    ("3/10 - step", [0, 0, 29, 9], 0, 0),
    ("3/10 + step", [0, 0, 30, 10], -1, -1),
    ("clear 0.9", [0, 0, 30, 27], 1, 1),
    ("clear 0.5", [0, 0, 30, 15], -1, -1),
    ("clear 0.1", [0, 0, 30, 3], 0, 0),
]


def rpn_threshold_case(variant):
    """gt [0,0,30,30] (area 900) has its exact copy as best anchor, so every other anchor is judged by the thresholds alone"""
    def seam(c, r):
        assert r.tab.row_value(1) == (T07 if variant == 1 else Fraction(630) / (900 + EPS_LAT))
        assert r.tab.row_value(4) == (T03 if variant == 1 else Fraction(270) / (900 + EPS_LAT))
        if variant == 0:
            assert r.tab.row_value(1) < T07 and r.tab.row_value(4) < T03
        assert r.pre.tolist() == [t[2 + (variant == 0)] for t in THRESH_ANCHORS]
    return RpnCase("thresholds-v%d" % variant, variant, [t[1] for t in THRESH_ANCHORS], [[0, 0, 30, 30]], seam)


G_ROUNDS = [1, 63, 64, 65, 128, 129, 4096]


def _many_boxes(G):
    """G distinct boxes inside the image: 256 corners x 16 sizes"""
    out = []
    for s in range(16):
        for y in range(16):
            for x in range(16):
                out.append([x, y, x + 13 + s % 4, y + 13 + s // 4])
    assert len({tuple(b) for b in out}) == len(out) >= G
    return out[:G]


def rpn_g_case(variant, G):
    """Every gt has its own unique best anchor, scattered over waves and workgroups.  G <= 129: slot gts whose best anchor has IoU 1/2,
    so only the per-gt rule makes it positive.  G = 4096 (64 rounds): 4096 distinct boxes, anchor = exact copy, N = G."""
    rng = np.random.RandomState(100 + G)
    if G == 4096:
        boxes = _many_boxes(G)
        order = rng.permutation(G)
        anchors = np.asarray(boxes, np.int64)[order]            # anchor i is the copy of gt order[i]

        def seam(c, r):
            assert c.G == 4096 and (r.col_count == 1).all() and np.array_equal(r.arg, order) and np.array_equal(r.col_first[order], np.arange(G))
        return RpnCase("G4096-v%d" % variant, variant, anchors, boxes, seam)
    N = 2600
    n_real = G - 1 if variant == 1 else G                       # variant 1: the blanket is the G-th gt
    where = _scatter(rng, N, n_real, fixed=[0, N - 1][:n_real])
    placed = {i: (slot_h(k) if k % 2 else slot_v(k)) for k, i in enumerate(where)}

    def seam(c, r):
        assert c.G == G and (r.col_count == 1).all()
        assert r.col_first[:n_real].tolist() == where and (r.pre[where] == 1).all() and r.n_pos == G
        assert all(r.tab.val_of_rank[m] < T07 for m in r.tab.col_max[:n_real])
        if n_real > 3:
            assert len({i // 1024 for i in where}) == 3 and len({i // 64 for i in where}) >= min(n_real, 41) // 2
    return assemble_rpn("G%d-v%d" % (G, variant), variant, N, placed, [slot_gt(k) for k in range(n_real)], seam)


N_SEAMS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 24575, 24576, 24577]


def rpn_n_case(variant, N):
    """anchor 0 and anchor N - 1 are each a gt's unique best (IoU 1/2)"""
    if N == 1:
        def seam1(c, r):
            assert c.N == 1 and r.pre.tolist() == [1]
        return RpnCase("N1-v%d" % variant, variant, [slot_h(0)], [slot_gt(0)], seam1)

    def seam(c, r):
        assert c.N == N and r.col_first[:2].tolist() == [0, N - 1] and (r.col_count == 1).all()
        assert r.pre[0] == 1 and r.pre[N - 1] == 1 and r.n_pos == (3 if variant == 1 else 2) and r.n_neg == 0
    return assemble_rpn("N%d-v%d" % (N, variant), variant, N, {0: slot_h(0), N - 1: slot_v(1)}, [slot_gt(0), slot_gt(1)], seam)


N_SAMPLED = [1023, 1024, 1025, 24575, 24576, 24577]


def rpn_n_sampled_case(variant, N):
    """the N seams with BOTH classes over quota, so that the sampler's sweep and its tail are on the line: anchors 0 and N - 1 are a gt's
    unique best, 150 exact copies of a third gt lie scattered (one at N - 3), every other anchor is a negative (N - 2 is one)."""
    rng = np.random.RandomState(N)
    big = [16, 16, 20, 20]
    where = _scatter(rng, N, 153, fixed=[0, N - 1, N - 3])
    anchors = np.asarray([_neg_box(k) for k in range(N)], np.int64)
    anchors[0], anchors[N - 1] = slot_h(0), slot_v(1)
    anchors[where[2:]] = big

    def seam(c, r):
        assert c.N == N and r.col_first[:2].tolist() == [0, N - 1] and (r.col_count[:2] == 1).all()
        assert (r.n_pos, r.n_neg) == (153, N - 153) and r.pre[N - 3] == 1 and r.pre[N - 2] == 0
    return RpnCase("N%d-sampled-v%d" % (N, variant), variant, anchors, [slot_gt(0), slot_gt(1), big], seam)


def rpn_quota_case(variant, n_pos, dneg):
    """n_pos positives (exact copies of one gt; variant 1 counts the blanket's copy among them) and 256 - min(n_pos, 128) + dneg negatives
    (unit squares that overlap no gt but, in variant 1, the blanket: IoU 1/1024)"""
    n_neg = 256 - min(n_pos, 128) + dneg
    N = 700
    rng = np.random.RandomState(7 * n_pos + dneg)
    n_copies = n_pos - 1 if variant == 1 else n_pos
    where = _scatter(rng, N, n_copies + n_neg)
    placed = {i: [0, 0, 16, 16] for i in where[:n_copies]}
    for j, i in enumerate(where[n_copies:]):
        placed[i] = [16 + j % 16, 16 + (j // 16) % 16, 17 + j % 16, 17 + (j // 16) % 16]

    def seam(c, r):
        assert (r.n_pos, r.n_neg) == (n_pos, n_neg)
    return assemble_rpn("quota-v%d-pos%d-neg%+d" % (variant, n_pos, dneg), variant, N, placed, [[0, 0, 16, 16]], seam)


def rpn_degenerate_case(variant, kind):
    """finite degenerate boxes.  No fillers and no blanket: every anchor is written out."""
    outside = [-8, 0, -4, 4]
    plain = [10, 10, 12, 12]                                     # overlaps no gt
    if kind == "lonely-gt":                                     # a gt that overlaps no anchor
        anchors, gts = [outside, plain, slot_h(0), slot_v(1)], [slot_gt(0), slot_gt(1), [30, 30, 32, 32]]
    elif kind == "zero-area-gt":                                # at index 1, so that it is nobody's first argmax and the targets stay finite
        anchors, gts = [outside, plain, slot_h(0), slot_v(1)], [slot_gt(0), [20, 20, 20, 24], slot_gt(1)]
    else:                                                       # "zero-area-anchor": IoU 0 with every gt; its targets divide by zero
        anchors, gts = [outside, slot_h(0), [10, 10, 10, 14], slot_v(1)], [slot_gt(0), slot_gt(1)]

    def seam(c, r):
        if kind == "zero-area-anchor":
            assert r.pre.tolist() == ([-1, 1, 0, 1] if variant == 0 else [0, 1, 0, 1])
            assert np.isinf(r.reg01[2, 0]) and np.isinf(r.reg23[2, 0])
        else:
            g = 2 if kind == "lonely-gt" else 1
            assert r.tab.val_of_rank[r.tab.col_max[g]] == 0
            # variant 0: the first anchor INSIDE the image; variant 1: every anchor with IoU 0 = every anchor
            assert r.pre.tolist() == ([-1, 1, 1, 1] if variant == 0 else [1, 1, 1, 1]) and r.col_first[g] == 1 - variant
            assert np.isfinite(r.reg23).all()
    return RpnCase("%s-v%d" % (kind, variant), variant, anchors, gts, seam)


def rpn_cases():
    out = []
    for v in (0, 1):
        out += [rpn_tie_case(v, False), rpn_tie_case(v, True), rpn_symmetric_tie_case(v), rpn_threshold_case(v)]
        out += [rpn_g_case(v, G) for G in G_ROUNDS]
        out += [rpn_n_case(v, N) for N in N_SEAMS] + [rpn_n_sampled_case(v, N) for N in N_SAMPLED]
        out += [rpn_quota_case(v, p, d) for p in (127, 128, 129) for d in (-1, 0, 1)]
        out += [rpn_degenerate_case(v, k) for k in ("lonely-gt", "zero-area-gt", "zero-area-anchor")]
    return out


_RPN, _HEAD = {}, {}


def rpn_case(name):
    if not _RPN:
        _RPN.update((c.name, c) for c in rpn_cases())
    return _RPN[name]


def rpn_case_names():
    rpn_case("N1-v0")
    return list(_RPN)


# ------------------------------------------------------------------------------------------------ head cases
HEAD_GT = [[0, 0, 10, 10], [12, 0, 22, 10], [0, 12, 10, 22]]     # three disjoint 10 x 10 gts; the region x, y >= 22 touches none of them
HEAD_LAB = [3, 7, 11]


def _pos_box(k):
    """a box with a clear IoU >= 0.5 to one gt (8/10 or 9/10, no tie): the gt shortened from its far side"""
    g = HEAD_GT[k % 3]
    return [g[0], g[1], g[2] - 1 - (k // 3) % 2, g[3]]


HEAD_N_SEAMS = [1023, 1024, 1025, 2048, 2049, 4095, 4096]


def head_count_case(variant, n, phase=0):
    """n = n_rois + G candidates.  Sparse positives around every round boundary (k = 1023, 1024, 2047, ...) and at the end; all other
    RoIs are negatives.  phase 1 shifts the positives by one, so that 1023 / 1024 swap roles."""
    G = len(HEAD_GT)
    P = n - G
    pos_at = sorted({k + phase for k in (0, 1022, 1024, 2046, 2048, 3070, 3072, P - 2) if 0 <= k + phase < P})
    rois = [_pos_box(k) if k in pos_at else _neg_box(k) for k in range(P)]

    def seam(c, r):
        assert c.n == n and r.pos_list.tolist() == pos_at + [P, P + 1, P + 2] and r.npc + r.nnc == n
        if n > 1025:
            assert (1023 in pos_at) != (1024 in pos_at)
        assert n - 1 in r.pos_list and (P - 1 in r.neg_list) == (phase == 0)
    return HeadCase("n%d-phase%d-v%d" % (n, phase, variant), variant, rois, HEAD_GT, HEAD_LAB, seam)


def head_device_count_case(variant):
    """a device n_rois below P_cap: rows behind it are never read, gt candidates are numbered from n_rois"""
    P_cap, n_rois = 1100, 1030
    rois = [_pos_box(k) if k % 97 == 0 else _neg_box(k) for k in range(P_cap)]

    def seam(c, r):
        assert c.rois.shape[0] == P_cap and c.n == n_rois + 3 and r.pos_list[-3:].tolist() == [n_rois, n_rois + 1, n_rois + 2]
        assert np.isnan(c.rois_f32()[n_rois:]).all() and not np.isnan(c.rois_f32()[:n_rois]).any()
    return HeadCase("device-count-v%d" % variant, variant, rois, HEAD_GT, HEAD_LAB, seam, n_rois=n_rois)


HEAD_THRESH = [
    ("1/2", [0, 0, 10, 20], True),                   # positive in variant 1, negative with eps
    ("1/2 + step", [0, 0, 10, 19], None),
    ("1/2 - step", [0, 0, 10, 21], None),
    ("touching: 0", [10, 0, 12, 10], None),
    ("one step in", [9, 0, 11, 10], None),
    ("one step away", [11, 0, 12, 10], None),
]


def head_threshold_case(variant):
    def seam(c, r):
        assert r.tab.row_value(0) == (T05 if variant == 1 else Fraction(100) / (200 + EPS_LAT))
        assert r.tab.row_value(3) == 0 and r.tab.row_value(5) == 0 and 0 < r.tab.row_value(4) < T05
        assert r.pos_list.tolist() == ([0, 1] if variant == 1 else [1]) + [6, 7, 8]
    return HeadCase("thresholds-v%d" % variant, variant, [t[1] for t in HEAD_THRESH], HEAD_GT, HEAD_LAB, seam, max_pos=4, total=8)


def head_argmax_tie_case(variant):
    """identical gt boxes with different labels at (g, g + 1) = (2, 3) and at (0, G - 1); two distinct gts (4, 5) with the same
    (inter, union) to a RoI.  The class is the lower g's."""
    gts = [[0, 0, 10, 10], [12, 0, 22, 10], [0, 12, 10, 22], [0, 12, 10, 22], [12, 12, 20, 24], [16, 12, 24, 24], [0, 0, 10, 10]]
    labs = [1, 2, 3, 4, 5, 6, 7]
    rois = [[0, 0, 10, 10], [0, 12, 10, 22], [14, 12, 22, 24], [0, 0, 10, 9], [0, 12, 10, 21]]

    def seam(c, r):
        assert r.arg[:5].tolist() == [0, 2, 4, 0, 2] and r.tab.row_tie_same.all() and r.npc == len(rois) + len(gts)
        uid, R = r.tab.block(0)
        assert R[0, 0] == R[0, 6] and R[1, 2] == R[1, 3] and R[2, 4] == R[2, 5] == r.tab.row_max[2] and uid[2, 4] == uid[2, 5]
        assert r.tab.row_value(2) > T05
    return HeadCase("argmax-ties-v%d" % variant, variant, rois, gts, labs, seam, max_pos=12, total=12)


def head_quota_case(variant, dpos, dneg):
    """npc = max_pos + dpos, nnc = total - n_pos + dneg.  (The three gts are positive candidates themselves.)"""
    c0 = HeadCase("", variant, [], HEAD_GT, HEAD_LAB, None)
    npc = c0.max_pos + dpos
    nnc = c0.total - min(npc, c0.max_pos) + dneg
    rng = np.random.RandomState(50 + 3 * dpos + dneg + 10 * variant)
    kinds = rng.permutation(np.array([1] * (npc - 3) + [0] * nnc))
    rois = [_pos_box(k) if kinds[k] else _neg_box(k) for k in range(len(kinds))]

    def seam(c, r):
        assert (r.npc, r.nnc) == (npc, nnc)
        rows = head_sample(c, np.arange(npc), np.arange(nnc))[4]
        assert (rows[2] < c.total) == (dneg < 0) and rows[3] == (HT_ERR_SHORT if dneg < 0 else 0)
    return HeadCase("quota-v%d-pos%+d-neg%+d" % (variant, dpos, dneg), variant, rois, HEAD_GT, HEAD_LAB, seam)


def head_row_limit_case(variant):
    """total = 1024 rows, all of them positives (max_pos = total)"""
    rois = [_pos_box(k) for k in range(1100)]

    def seam(c, r):
        assert c.total == 1024 == c.max_pos and r.npc == 1103 and r.nnc == 0
    return HeadCase("rows1024-v%d" % variant, variant, rois, HEAD_GT, HEAD_LAB, seam, max_pos=1024, total=1024)


def head_cases():
    out = []
    for v in (0, 1):
        out += [head_count_case(v, n) for n in HEAD_N_SEAMS] + [head_count_case(v, 1024, 1), head_count_case(v, 1025, 1)]
        out += [head_device_count_case(v), head_threshold_case(v), head_argmax_tie_case(v), head_row_limit_case(v)]
        out += [head_quota_case(v, dp, dn) for dp in (-1, 0, 1) for dn in (-1, 0, 1)]
    return out


def head_case(name):
    if not _HEAD:
        _HEAD.update((c.name, c) for c in head_cases())
    return _HEAD[name]


def head_case_names():
    head_case("thresholds-v0")
    return list(_HEAD)


def head_perms(case, kind):
    """the host permutations the tests run a head case with"""
    r = head_match(case)
    if kind == "identity":
        return np.arange(r.npc), np.arange(r.nnc)
    if kind == "reversed":
        return np.arange(r.npc)[::-1].copy(), np.arange(r.nnc)[::-1].copy()
    rng = np.random.RandomState(r.npc * 7 + r.nnc)
    return rng.permutation(r.npc), rng.permutation(r.nnc)


def rpn_perms(case, seed=0):
    """random host permutations, drawn only where the reference draws them"""
    r = rpn_match(case)
    rng = np.random.RandomState(seed + r.n_pos + 3 * r.n_neg)
    pp = rng.permutation(r.n_pos) if r.n_pos > 128 else None
    pn = rng.permutation(r.n_neg) if r.n_neg > 256 - r.n_pos else None
    return pp, pn
