"""numpy restatement of frcnn_detect_merge_soft's contract (include/frcnn_hip.h): the merge of detection sets with Soft-NMS (Bodla et
al., 2017) as its suppression step, fp32 operation by operation (`soft_merge`), and a second, independent restatement of the scan that
transcribes the loop Detectron published (swap the maximum to the front, decay the tail, swap a dropped box to the end; `literal=True`).
Everything around the scan -- flips, IoU, voting sums, test data -- is detect_merge_ref's.  Not a test module: test_soft_nms_host.py
and test_gpu_soft_nms.py import it."""
import numpy as np

from detect_merge_ref import (CLASS_OVERFLOW, COUNT_CLIPPED, LABEL_RANGE, MAX_CANDIDATES, OUTPUT_OVERFLOW, UPSTREAM_ABORT, area, dyadic_cluster,  # noqa: F401
                              flip, iou, random_sets, same_bits, vote)

HARD, LINEAR, GAUSSIAN = 0, 1, 2
F = np.float32


def _gap(a, b):
    """The relative gap of two scores; inf when it says nothing (a non-finite operand)."""
    a, b = float(a), float(b)
    if not (np.isfinite(a) and np.isfinite(b)):
        return np.inf
    d = max(abs(a), abs(b))
    return abs(a - b) / d if d > 0 else 0.0


def _decay(w, ov, method, nms_thr, sigma):
    """(decayed scores, which were decayed) of the fp32 arrays w and ov."""
    with np.errstate(all="ignore"):
        if method == LINEAR:
            hit = ov > F(nms_thr)
            return np.where(hit, w * (F(1.0) - ov), w).astype(F), hit
        hit = ov > F(0.0)
        o = ov.astype(np.float64)
        wt = np.exp(-(o * o) / np.float64(F(sigma))).astype(F)                # the weight in binary64, rounded once
        return np.where(hit, w * wt, w).astype(F), hit


def soft_class(boxes, scores, method, nms_thr, sigma, floor):
    """One class, candidates in sorted order: (emitted positions, their working scores, the decays each received, the margin)."""
    m = len(scores)
    A = area(boxes)
    w = np.array(scores, F, copy=True)
    live = np.ones(m, bool)
    nd = np.zeros(m, np.int64)
    kept, ks, margin = [], [], np.inf
    while live.any():
        idx = np.flatnonzero(live)
        wl = w[idx] + F(0.0)                                                   # -0 counts as +0
        best = idx[int(np.argmax(wl))]                                         # the first maximum: the smallest position
        if len(idx) > 1:
            margin = min(margin, _gap(w[best], np.max(np.delete(wl, int(np.argmax(wl))))))
        kept.append(best)
        ks.append(w[best])
        live[best] = False
        ov = iou(boxes[best], A[best], boxes, A)
        with np.errstate(all="ignore"):
            if method == HARD:
                live &= ~(ov > F(nms_thr))
                continue
            nw, hit = _decay(w, ov, method, nms_thr, sigma)
            hit &= live
            w = np.where(hit, nw, w).astype(F)
            nd += hit
            for j in np.flatnonzero(hit):
                margin = min(margin, _gap(w[j], F(floor)))
            live &= ~(hit & ~(w >= F(floor)))                                  # a NaN drops
    return np.array(kept, np.int64), np.array(ks, F), nd[kept] if kept else np.zeros(0, np.int64), margin


def soft_class_literal(boxes, scores, method, nms_thr, sigma, floor):
    """The same scan as Detectron's cpu_soft_nms writes it: one array of rows that is permuted in place.  Row i .. N-1 are live; the
    maximum of the tail is swapped to i, the tail is decayed against it, a row that falls under the floor is overwritten by the last row and
    N shrinks.  The IoU is this project's, the tie between equal scores goes to the smaller sorted position (the published loop keeps
    whichever comes first in its permuted array), and only a decayed row meets the floor -- the contract's words."""
    N = len(scores)
    A = area(boxes)
    rows = [[p, F(scores[p]), 0] for p in range(N)]                            # sorted position, working score, decays
    i = 0
    with np.errstate(all="ignore"):
        while i < N:
            maxpos = i
            for pos in range(i + 1, N):
                a, b = rows[pos][1] + F(0.0), rows[maxpos][1] + F(0.0)
                if b < a or (a == b and rows[pos][0] < rows[maxpos][0]):
                    maxpos = pos
            rows[i], rows[maxpos] = rows[maxpos], rows[i]
            pi = rows[i][0]
            pos = i + 1
            while pos < N:
                pj = rows[pos][0]
                ov = iou(boxes[pi], A[pi], boxes[pj:pj + 1], A[pj:pj + 1])[0]
                drop = False
                if method == HARD:
                    drop = bool(ov > F(nms_thr))
                elif (ov > F(nms_thr)) if method == LINEAR else (ov > F(0.0)):
                    if method == LINEAR:
                        weight = F(F(1.0) - ov)
                    else:
                        weight = F(np.exp(-(np.float64(ov) * np.float64(ov)) / np.float64(F(sigma))))
                    rows[pos][1] = F(rows[pos][1] * weight)
                    rows[pos][2] += 1
                    drop = not bool(rows[pos][1] >= F(floor))
                if drop:
                    rows[pos] = rows[N - 1]
                    N -= 1
                    pos -= 1
                pos += 1
            i += 1
    rows = rows[:N]
    return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], F), np.array([r[2] for r in rows], np.int64), np.inf)


def soft_merge(sets, flags, C, method, nms_thr=0.3, sigma=0.5, floor=1e-3, min_score=0.0, vote_thr=None, out_capacity=None, literal=False):
    """sets: K tuples (boxes [cap,4] f32, labels [cap] i32, scores [cap] f32, count int).  Returns detect_merge_ref.merge's dict -- boxes /
    labels / scores of the first `total` rows (class-major; the scores are the working scores), count, class_counts, status, unvoted -- and
    decays (per emitted box, the number of decays it received) and margin (the smallest relative gap, over all steps, between the picked
    working score and the runner-up's and between a decayed score and the floor: how far the run is from taking another turn)."""
    status = 0
    cand = [[] for _ in range(C - 1)]                                          # per class: (folded score, set, row)
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
                cand[l[r]].append((-float(s[r]) + 0.0, k, r))
    scan = soft_class_literal if literal else soft_class
    ob, ol, os_, ub, cc, decays, margin = [], [], [], [], [], [], np.inf
    for c in range(C - 1):
        order = sorted(cand[c])
        if len(order) > MAX_CANDIDATES:
            status |= CLASS_OVERFLOW
            order = []
        boxes = np.array([tb[k][r] for _, k, r in order], F).reshape(-1, 4)
        scores = np.array([sets[k][2][r] for _, k, r in order], F)
        kept, ks, nd, mg = scan(boxes, scores, method, nms_thr, sigma, floor)
        margin = min(margin, mg)
        out = boxes[kept].copy() if len(kept) else np.zeros((0, 4), F)
        if vote_thr is not None and vote_thr >= 0:
            A = area(boxes)
            for q, i in enumerate(kept):
                with np.errstate(all="ignore"):
                    voters = iou(boxes[i], A[i], boxes, A) >= F(vote_thr)
                voters[i] = True
                out[q] = vote(boxes, scores, i, voters)                        # weighted by the ORIGINAL scores
        ob.append(out)
        ub.append(boxes[kept].reshape(-1, 4))
        os_.append(ks)
        ol.append(np.full(len(kept), c, np.int32))
        cc.append(len(kept))
        decays.append(nd)
    total = int(sum(cc))
    if out_capacity is None:
        out_capacity = total
    if total > out_capacity:
        status |= OUTPUT_OVERFLOW
    count = -1 if status & (UPSTREAM_ABORT | CLASS_OVERFLOW | OUTPUT_OVERFLOW) else total
    return dict(boxes=np.concatenate(ob).astype(F).reshape(-1, 4), labels=np.concatenate(ol).astype(np.int32), scores=np.concatenate(os_).astype(F),
                unvoted=np.concatenate(ub).astype(F).reshape(-1, 4), count=count, total=total, class_counts=np.array(cc, np.int32), status=status,
                decays=np.concatenate(decays).astype(np.int64), margin=margin)


# ---- test data, shared by the host and the GPU tests ----
def one_class(rng, m, spread=0.08):
    """One set, one class (C = 2), m live rows around four objects."""
    b, l, s, n = random_sets(rng, 1, 2, [m], [m], spread=spread)[0]
    return [(b, l, s, n)]


def gaussian_cases():
    """The inputs of the GPU tests of gaussian mode, at most 64 candidates per class: (name, sets, flags, C, keyword arguments of
    soft_merge).  test_soft_nms_host.py holds the margin of every one above 1e-4, so that rounding differences of the device's binary64
    exp cannot turn a pick or a floor decision, and the GPU comparison leaves out no case."""
    cases = []
    for name, seed, K, C, per, kw in [("K1_C2", 31, 1, 2, 60, dict(sigma=0.5)),
                                      ("K2_C3", 32, 2, 3, 50, dict(sigma=0.5)),
                                      ("K3_C5_sigma03", 33, 3, 5, 60, dict(sigma=0.3, floor=0.05)),
                                      ("K2_C3_vote", 34, 2, 3, 50, dict(sigma=0.5, vote_thr=0.8)),
                                      ("K2_C4_flip", 35, 2, 4, 70, dict(sigma=0.7, floor=0.01))]:
        rng = np.random.RandomState(seed)
        sets = random_sets(rng, K, C, [per + 5 + k for k in range(K)], [per - k for k in range(K)], spread=0.15)
        flags = [0, 1, 2][:K]
        sets = [(flip(b, f), l, s, n) for (b, l, s, n), f in zip(sets, flags)]  # stored mirrored, so that the merge brings them back
        cases.append((name, sets, flags, C, kw))
    return cases
