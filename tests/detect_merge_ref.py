"""numpy restatement of frcnn_detect_merge's contract (include/frcnn_hip.h): fp32 arithmetic op by op, the voting sums in the
lane-strided order and the xor butterfly the header states (`merge`), and a second, naive form of the voting (np.average in float64,
`naive=True`) that must agree with the literal one on exact (dyadic) data.  Not a test module: test_detect_merge_host.py and
test_gpu_detect_merge.py import it."""
import numpy as np

COUNT_CLIPPED, UPSTREAM_ABORT, LABEL_RANGE, CLASS_OVERFLOW, OUTPUT_OVERFLOW = 1, 2, 4, 8, 16
MAX_CANDIDATES = 2048
F = np.float32


def flip(boxes, flags):
    """flags bit 0: (1 - x2, y1, 1 - x1, y2); bit 1: the same for y.  One fp32 subtraction each."""
    b = np.array(boxes, F, copy=True).reshape(-1, 4)
    one = F(1.0)
    if flags & 1:
        b[:, 0], b[:, 2] = one - b[:, 2], one - b[:, 0]
    if flags & 2:
        b[:, 1], b[:, 3] = one - b[:, 3], one - b[:, 1]
    return b


def area(b):
    b = np.asarray(b, F)
    return (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])


def iou(bi, ai, B, A):
    """nms_dev.h's expression in fp32: max / min that return the other operand for a NaN one (v_max_f32 / v_min_f32)."""
    with np.errstate(all="ignore"):
        w = np.fmax(np.fmin(bi[2], B[:, 2]) - np.fmax(bi[0], B[:, 0]), F(0))
        h = np.fmax(np.fmin(bi[3], B[:, 3]) - np.fmax(bi[1], B[:, 1]), F(0))
        inter = (w * h).astype(F)
        return (inter / ((ai + A).astype(F) - inter).astype(F)).astype(F)


def _vote_literal(s, x, voters):
    """sum_j s_j x_j over the voters in the header's order: lane l adds the sorted positions p = l (mod 64) in ascending p onto +0.0, the
    64 partials are combined by the butterfly with offsets 32 .. 1.  s, x float64 [m]; returns lane 0's value (every lane holds the same)."""
    m = len(s)
    with np.errstate(all="ignore"):
        term = np.where(voters, s * x, 0.0)                    # a non-voter adds nothing: +0.0 leaves a partial that started at +0.0 as it is
        rows = -(-m // 64)
        pad = np.zeros(rows * 64, np.float64)
        pad[:m] = term
        acc = np.zeros(64, np.float64)
        for r in range(rows):
            acc = acc + pad[64 * r:64 * r + 64]
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lanes ^ o]
    return acc[0]


def vote(boxes, scores, pi, voters, naive=False):
    """The voted box of the kept candidate at sorted position pi; its original bits when it is its own only voter, a sum is not finite or
    the weight sum is not > 0."""
    if int(voters.sum()) <= 1:
        return boxes[pi].copy()
    s = scores.astype(np.float64)
    b = boxes.astype(np.float64)
    with np.errstate(all="ignore"):
        if naive:
            sw = s[voters].sum()
            sums = (b[voters] * s[voters, None]).sum(0)
            if not (np.isfinite(sw) and np.isfinite(sums).all() and sw > 0):
                return boxes[pi].copy()
            return np.average(b[voters], axis=0, weights=s[voters]).astype(F)
        sw = _vote_literal(s, np.ones_like(s), voters)
        sums = np.array([_vote_literal(s, b[:, c], voters) for c in range(4)])
        if not (np.isfinite(sw) and np.isfinite(sums).all() and sw > 0):
            return boxes[pi].copy()
        return (sums / sw).astype(F)


def merge_class(boxes, scores, nms_thr, vote_thr, naive=False):
    """One class: candidates already in (score desc, set asc, row asc) order and transformed.  Returns (kept positions, kept boxes after
    voting, info) with info = (suppressed candidates, the voter count of every kept box)."""
    m = len(scores)
    A = area(boxes)
    sup = np.zeros(m, bool)
    kept = []
    for i in range(m):
        if sup[i]:
            continue
        kept.append(i)
        if i + 1 < m:
            with np.errstate(all="ignore"):
                sup[i + 1:] |= iou(boxes[i], A[i], boxes[i + 1:], A[i + 1:]) > F(nms_thr)
    out = boxes[kept].copy() if kept else np.zeros((0, 4), F)
    nvoters = []
    if vote_thr is not None and vote_thr >= 0:
        for q, i in enumerate(kept):
            with np.errstate(all="ignore"):
                voters = iou(boxes[i], A[i], boxes, A) >= F(vote_thr)
            voters[i] = True
            nvoters.append(int(voters.sum()))
            out[q] = vote(boxes, scores, i, voters, naive)
    return np.array(kept, np.int64), out, (int(sup.sum()), nvoters)


def merge(sets, flags, C, min_score=0.0, nms_thr=0.3, vote_thr=None, out_capacity=None, naive=False):
    """sets: K tuples (boxes [cap,4] f32, labels [cap] i32, scores [cap] f32, count int).  Returns a dict: boxes / labels / scores of the
    first `total` rows (class-major), count (-1 as the header says), class_counts [C-1], status, and for the tests' own checks: unvoted (the
    kept boxes before voting), suppressed, voters (per kept box; empty without voting)."""
    status = 0
    cand = [[] for _ in range(C - 1)]                          # per class: (folded score, set, row)
    tb = []
    for k, (b, l, s, n) in enumerate(sets):
        b, l, s = np.asarray(b, F).reshape(-1, 4), np.asarray(l, np.int32), np.asarray(s, F)
        cap = len(l)
        tb.append(flip(b, flags[k]))
        if n < 0:
            status |= UPSTREAM_ABORT
            n = 0
        elif n > cap:
            status |= COUNT_CLIPPED
            n = cap
        for r in range(n):
            if not 0 <= l[r] < C - 1:
                status |= LABEL_RANGE
                continue
            if s[r] > F(min_score):
                cand[l[r]].append((-float(s[r]) + 0.0, k, r))  # -0 and +0 compare equal; (set, row) break ties
    ob, ol, os_, ub, cc, nsup, voters = [], [], [], [], [], 0, []
    for c in range(C - 1):
        order = sorted(cand[c])
        if len(order) > MAX_CANDIDATES:
            status |= CLASS_OVERFLOW
            order = []
        boxes = np.array([tb[k][r] for _, k, r in order], F).reshape(-1, 4)
        scores = np.array([sets[k][2][r] for _, k, r in order], F)
        kept, vb, (ns, nv) = merge_class(boxes, scores, nms_thr, vote_thr, naive)
        ob.append(vb)
        ub.append(boxes[kept])
        os_.append(scores[kept])
        ol.append(np.full(len(kept), c, np.int32))
        cc.append(len(kept))
        nsup += ns
        voters += nv
    total = int(sum(cc))
    if out_capacity is None:
        out_capacity = total
    if total > out_capacity:
        status |= OUTPUT_OVERFLOW
    count = -1 if status & (UPSTREAM_ABORT | CLASS_OVERFLOW | OUTPUT_OVERFLOW) else total
    return dict(boxes=np.concatenate(ob).astype(F).reshape(-1, 4), labels=np.concatenate(ol).astype(np.int32), scores=np.concatenate(os_).astype(F),
                unvoted=np.concatenate(ub).astype(F).reshape(-1, 4), count=count, total=total, class_counts=np.array(cc, np.int32), status=status,
                suppressed=nsup, voters=voters)


# ---- test data, shared by the host and the GPU tests ----
def random_sets(rng, K, C, caps, counts, dyadic=False, spread=0.08):
    """K sets around a few shared objects per class, so that views overlap: boxes in [0, 1], scores in (0, 1)."""
    n_obj = 4
    centres = rng.rand(C - 1, n_obj, 2) * 0.6 + 0.2
    sizes = rng.rand(C - 1, n_obj, 2) * 0.2 + 0.1
    out = []
    for k in range(K):
        cap = caps[k]
        lab = rng.randint(0, C - 1, cap).astype(np.int32)
        o = rng.randint(0, n_obj, cap)
        c = centres[lab, o] + (rng.rand(cap, 2) - 0.5) * spread
        wh = sizes[lab, o] * (1 + (rng.rand(cap, 2) - 0.5) * spread * 4)
        b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1)
        s = rng.rand(cap) * 0.9 + 0.05
        if dyadic:
            b, s = np.round(b * 64) / 64, np.round(s * 16 + 1) / 32
        out.append((b.astype(F), lab, s.astype(F), counts[k]))
    return out


def dyadic_cluster(rng, m):
    """One class, m mutually overlapping candidates (IoU > 0.5 each with each) on a 1/256 grid, scores k/64: every product and sum exact."""
    j = rng.randint(0, 8, (m, 4))
    b = (np.array([64, 64, 192, 192]) + j * np.array([1, 1, -1, -1])) / 256.0
    s = rng.randint(1, 64, m) / 64.0
    return [(b.astype(F), np.zeros(m, np.int32), s.astype(F), m)]


def same_bits(a, b):
    """Equal shapes and every value bit-identical (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
