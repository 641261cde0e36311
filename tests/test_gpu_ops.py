"""Parity tests proper: HIP kernels (through the C ABI, via faster_rcnn_pytorch_amd.ops) vs the CPU oracle
on identical seeded inputs.  Integer results must be bit-exact; floating point as stated per test.
Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def rand_boxes(rng, n, lo=0.02, hi=0.6):
    c = rng.rand(n, 2) * 0.8 + 0.1
    wh = rng.rand(n, 2) * (hi - lo) + lo
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


def rpn_outputs(rng, N, regime):
    """SURVEY 8d synthetic RPN outputs: init-like / trained-like."""
    if regime == "init":
        reg = (rng.randn(N, 4) * 0.02).astype(np.float32)
        cls = (rng.randn(N, 2) * 0.02).astype(np.float32)
    else:
        reg = (rng.randn(N, 4) * np.array([0.1, 0.1, 0.2, 0.2])).astype(np.float32)
        d = (rng.randn(N) * 2 - 2).astype(np.float32)
        cls = np.stack([np.zeros(N, np.float32), d], 1)
    return reg, cls


# ------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize("hw", [(600, 1000), (800, 800), (37, 50), (880, 960)])
def test_anchor_grid_vgg_bit_exact(ops, hw):
    H, W = hw
    base = ops.anchor_base()
    assert np.array_equal(base, orc.anchor_base())
    got = ops.anchor_grid([(H // 16, W // 16)], [(16, 16)], base[None], W, H, DEV).cpu().numpy()
    assert np.array_equal(got, orc.anchor_grid(H, W))


def test_anchor_grid_fpn_bit_exact(ops, golden):
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    ag = ops.AnchorGenerator()
    px = ag.grid((800, 1344), shapes, DEV).cpu().numpy()
    assert np.array_equal(px, orc.tv_anchor_grid(800, 1344, shapes, normalise=False))
    nm = ag.grid((800, 1344), shapes, DEV, normalise=True).cpu().numpy()
    assert np.array_equal(nm, orc.tv_anchor_grid(800, 1344, shapes, normalise=True))
    assert nm.shape == (268569, 4)


# ------------------------------------------------------------------------------------------ codec / IoU
def test_codec_vs_oracle_and_golden(ops, golden):
    g = golden("codec")
    assert np.array_equal(ops.xy_to_cxcy(T(g["xy"])).cpu().numpy(), g["xy_to_cxcy"])
    assert np.array_equal(ops.cxcy_to_xy(T(g["xy_to_cxcy"])).cpu().numpy(), g["cxcy_to_xy"])
    dec = ops.decode(T(g["t"]), T(g["anc_cxcy"])).cpu().numpy()
    assert np.array_equal(dec, orc.decode(g["t"], g["anc_cxcy"]), equal_nan=True)          # bit-exact vs oracle (deterministic exp)
    fin = np.isfinite(g["decode"])
    assert (np.abs(dec[fin] - g["decode"][fin]) <= 4e-7 * np.abs(g["decode"][fin])).all()   # vs reference torch.exp
    enc = ops.encode(T(g["gt_cxcy"]), T(g["anc_cxcy"])).cpu().numpy()
    assert np.array_equal(enc[:, :2], g["encode"][:, :2])
    assert np.abs(enc[:, 2:] - g["encode"][:, 2:]).max() < 1e-6                             # logf: tolerance 1e-6 (north star: 1e-4)


def test_pairwise_iou_bit_exact(ops, golden):
    g = golden("codec")
    got = ops.find_jaccard_overlap(T(g["s1"]), T(g["s2"])).cpu().numpy()
    assert np.array_equal(got, g["jaccard"])                                               # reference vector
    rng = np.random.RandomState(0)
    a, b = rand_boxes(rng, 3000), rand_boxes(rng, 11)
    assert np.array_equal(ops.find_jaccard_overlap(T(a), T(b)).cpu().numpy(), orc.pairwise_iou(a, b, 1e-5))
    iou, union = ops.box_iou(T(b), T(a))
    assert np.array_equal(iou.cpu().numpy(), orc.pairwise_iou(b, a, 0.0))
    assert union.shape == (11, 3000)


# ------------------------------------------------------------------------------------------ prologue
@pytest.mark.parametrize("regime", ["init", "trained"])
def test_prologue_bit_exact(ops, regime):
    rng = np.random.RandomState(1)
    anchor = orc.anchor_grid(600, 1000)
    N = anchor.shape[0]
    reg, cls = rpn_outputs(rng, N, regime)
    reg[::97, 2:] = -12.0                                   # collapse some boxes below min_size
    reg[5, 2] = 120.0                                       # exp overflow -> inf -> clamp
    b_o, s_o, nv = orc.proposal_prologue(reg, cls, anchor, 1 / 1000)
    b_g, s_g = ops.proposal_prologue(T(reg), T(cls), T(anchor), 1 / 1000)
    assert np.array_equal(b_g.cpu().numpy(), b_o, equal_nan=True)
    assert np.array_equal(s_g.cpu().numpy(), s_o)
    assert int((s_g >= 0).sum()) == nv and nv < N


def test_prologue_matches_reference_golden(ops, golden):
    g = golden("proposal_pre_nms")
    b, s = ops.proposal_prologue(T(g["reg"]), T(g["cls"]), T(g["anchor"]), 1 / 1000)
    b, s = b.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(s >= 0, g["keep"])
    assert np.abs(b - g["roi_all"]).max() < 1e-6                                             # tolerance 1e-6 << 1e-4
    assert np.abs(s[g["keep"]] - g["score_all"][g["keep"]]).max() < 2e-7


# ------------------------------------------------------------------------------------------ top-k
@pytest.mark.parametrize("N,K", [(20646, 12000), (20646, 6000), (1000, 1000), (777, 2000), (65, 64), (1, 1),
                                 (268569, 4000), (268569, 2000), (100000, 2000), (40000, 10000)])   # last four: radix-select pre-filter path
def test_topk_bit_exact(ops, N, K):
    rng = np.random.RandomState(N + K)
    s = rng.rand(N).astype(np.float32)
    s[rng.rand(N) < 0.1] = -1.0                             # filtered
    boxes = rand_boxes(rng, N)
    idx_o, sc_o = orc.topk_sorted(s, K)
    idx, sc, bx, cnt = ops.topk_sorted(T(s), K, T(boxes))
    n = int(cnt.item())
    assert n == len(idx_o)
    assert np.array_equal(idx[:n].cpu().numpy(), idx_o)
    assert np.array_equal(sc[:n].cpu().numpy(), sc_o)
    assert np.array_equal(bx[:n].cpu().numpy(), boxes[idx_o])


def test_topk_large_n_with_heavy_ties_and_few_valid(ops):
    rng = np.random.RandomState(3)
    N = 150000
    s = (rng.randint(0, 2000, N) / 4096.0).astype(np.float32)      # ~75 equal scores per value: the candidate band is wide
    s[::7] = -1.0
    idx_o, sc_o = orc.topk_sorted(s, 3000)
    idx, sc, _, cnt = ops.topk_sorted(T(s), 3000)
    assert int(cnt.item()) == 3000 and np.array_equal(idx.cpu().numpy(), idx_o) and np.array_equal(sc.cpu().numpy(), sc_o)
    few = np.full(N, -1.0, np.float32)                              # fewer valid entries than K
    pos = rng.choice(N, 500, replace=False)
    few[pos] = rng.rand(500).astype(np.float32)
    idx_o, _ = orc.topk_sorted(few, 3000)
    idx, _, _, cnt = ops.topk_sorted(T(few), 3000)
    assert int(cnt.item()) == 500 and np.array_equal(idx[:500].cpu().numpy(), idx_o)


def test_topk_above_the_coresident_grid_limit(ops):
    """N > 1 048 576 scores: the partition's grid (N / 1024 workgroups) is above what the launcher treats as certainly co-resident, so
    the sample sort takes its barrier-free three-launch form (topk_count / topk_place / topk_bucket) by itself."""
    rng = np.random.RandomState(8)
    N, K = 1_100_000, 5000
    s = rng.rand(N).astype(np.float32)
    s[rng.rand(N) < 0.2] = -1.0
    order = np.lexsort((np.arange(N), -s.astype(np.float64)))[:K]          # score descending, index ascending
    idx, sc, _, cnt = ops.topk_sorted(T(s), K)
    assert int(cnt.item()) == K
    assert np.array_equal(idx.cpu().numpy(), order) and np.array_equal(sc.cpu().numpy(), s[order])


def test_topk_ties_resolve_by_index(ops):
    rng = np.random.RandomState(7)
    N = 5000
    s = (rng.randint(0, 40, N) / 64.0).astype(np.float32)   # heavy ties
    s[::11] = -1.0
    idx_o, _ = orc.topk_sorted(s, 3000)
    idx, _, _, cnt = ops.topk_sorted(T(s), 3000)
    assert int(cnt.item()) == 3000 and np.array_equal(idx.cpu().numpy(), idx_o)
    same = np.full(300, 0.5, np.float32)                    # all equal (zero-init RPN): identity order
    idx, _, _, cnt = ops.topk_sorted(T(same), 200)
    assert np.array_equal(idx.cpu().numpy(), np.arange(200))
    allbad = np.full(300, -1.0, np.float32)
    _, _, _, cnt = ops.topk_sorted(T(allbad), 200)
    assert int(cnt.item()) == 0


# ------------------------------------------------------------------------------------------ NMS
def test_nms_known_answers(ops):
    def run(b, thr):
        b = np.asarray(b, np.float32)
        sc = np.linspace(1.0, 0.5, len(b)).astype(np.float32)
        return ops.nms(T(b), T(sc), thr).cpu().tolist()
    b = [[0, 0, 1, 1], [0.5, 0, 1.5, 1], [2, 2, 3, 3]]
    assert run(b, 0.3) == [0, 2] and run(b, 0.34) == [0, 1, 2]
    b2 = [[0, 0, 2, 1], [0, 0, 1, 1]]                       # IoU exactly 0.5: strict > keeps both
    assert run(b2, 0.5) == [0, 1]
    assert run(b2, float(np.nextafter(np.float32(0.5), np.float32(0)))) == [0]
    c = [[0, 0, 1, 1], [0.2, 0, 1.2, 1], [0.4, 0, 1.4, 1]]  # 0 kills 1, so 1 cannot kill 2
    assert run(c, 0.5) == [0, 2]
    z = [[0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5]]        # 0/0 = NaN is not > thr
    assert run(z, 0.1) == [0, 1]


def test_nms_sorts_by_score_like_torchvision(ops):
    b = np.array([[0, 0, 1, 1], [0.1, 0, 1.1, 1], [2, 2, 3, 3]], np.float32)
    sc = np.array([0.2, 0.9, 0.5], np.float32)
    assert ops.nms(T(b), T(sc), 0.5).cpu().tolist() == [1, 2]
    order = np.argsort(-sc, kind="stable")
    assert orc.nms(b, 0.5, order=order).tolist() == [1, 2]


@pytest.mark.parametrize("K,thr", [(12000, 0.7), (6000, 0.7), (4000, 0.7), (1000, 0.3), (777, 0.5), (64, 0.5), (65, 0.5), (3, 0.5)])
def test_nms_bit_exact_vs_oracle(ops, K, thr):
    rng = np.random.RandomState(K)
    c = rng.rand(K, 2).astype(np.float32) * 0.7 + 0.15
    wh = (rng.rand(K, 2).astype(np.float32) * 0.25 + 0.03)
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    keep_o = orc.nms(b, thr)
    keep, rois, cnt = ops.nms_sorted(T(b), thr, want_rois=True)
    n = int(cnt.item())
    assert n == len(keep_o)
    assert np.array_equal(keep[:n].cpu().numpy(), keep_o)
    assert np.array_equal(rois[:n].cpu().numpy(), b[keep_o])
    # post_k early exit + live count on the device
    post = max(1, len(keep_o) // 3)
    keep, _, cnt = ops.nms_sorted(T(b), thr, post_k=post)
    assert int(cnt.item()) == post and np.array_equal(keep[:post].cpu().numpy(), keep_o[:post])
    live = max(1, K - 37)
    keep, _, cnt = ops.nms_sorted(T(b), thr, n_boxes=T(np.array([live], np.int32)))
    ko = orc.nms(b[:live], thr)
    assert int(cnt.item()) == len(ko) and np.array_equal(keep[:len(ko)].cpu().numpy(), ko)


def _spread_boxes(rng, K, lo=0.05, hi=0.35):
    c = rng.rand(K, 2).astype(np.float32) * 0.7 + 0.15
    wh = (rng.rand(K, 2).astype(np.float32) * (hi - lo) + lo)
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)


CASCADE_K = 20000              # > NMS_CASCADE_MIN = 16 384 (csrc/nms.hip): the two-level cascade is what runs, in the default environment


@pytest.mark.parametrize("live", [1, 64, 1500, 2047, 2048, 2049, 2111, 2112, 2113, 4097, 16383, 16384, 16385, 19967, 19968, 19969, 19999, 20000])
def test_nms_cascade_live_count_around_the_level_boundary(ops, live):
    """K = 20 000 > NMS_CASCADE_MIN takes the cascade (top NMS_T_MAX = 2048 -> nms_filter_kernel -> survivors through nms_kernel again
    -> two-level nms_emit_kernel); the device-side live count may fall anywhere relative to the level boundary (2048), the second level's
    64-box block boundaries and the end of the buffer, including an empty second level.  Keep lists, rois and counts vs the oracle."""
    rng = np.random.RandomState(5)
    K = CASCADE_K
    b = _spread_boxes(rng, K)
    ko = orc.nms(b[:live], 0.7)
    keep, rois, cnt = ops.nms_sorted(T(b), 0.7, n_boxes=T(np.array([live], np.int32)), want_rois=True)
    n = int(cnt.item())
    assert n == len(ko) and np.array_equal(keep[:n].cpu().numpy(), ko) and np.array_equal(rois[:n].cpu().numpy(), b[ko])
    n0 = int((ko < 2048).sum())                                   # kept boxes of level 0
    for post in sorted({1, max(1, n0 // 2), max(1, n0 - 1), max(1, n0), min(len(ko), n0 + 1), max(1, (n0 + len(ko)) // 2), len(ko)}):
        keep, _, cnt = ops.nms_sorted(T(b), 0.7, post_k=post, n_boxes=T(np.array([live], np.int32)))   # post_k cuts inside level 0 / at the seam / inside level 1
        assert int(cnt.item()) == post and np.array_equal(keep[:post].cpu().numpy(), ko[:post]), post


@pytest.mark.parametrize("K,thr", [(16385, 0.7), (20000, 0.7), (20000, 0.3), (40000, 0.5), (40000, 0.7)])
def test_nms_cascade_keep_lists_vs_oracle(ops, K, thr):
    """keep LISTS (not counts) of the cascade at the sizes FRCNN.predict's class-aware lists reach (up to
    1000 x 90 candidates, new_model.py _suppress), through every entry point: nms_sorted, nms (sorts by score first), batched_nms."""
    rng = np.random.RandomState(K + int(thr * 10))
    b = _spread_boxes(rng, K, 0.03, 0.28)
    ko = orc.nms(b, thr)
    keep, rois, cnt = ops.nms_sorted(T(b), thr, want_rois=True)
    n = int(cnt.item())
    assert n == len(ko) and np.array_equal(keep[:n].cpu().numpy(), ko) and np.array_equal(rois[:n].cpu().numpy(), b[ko])
    sc = ((rng.permutation(K) + 1) / np.float32(K + 1)).astype(np.float32)       # distinct scores: the order is unambiguous
    assert len(np.unique(sc)) == K
    order = np.argsort(-sc, kind="stable")
    assert np.array_equal(ops.nms(T(b), T(sc), thr).cpu().numpy(), orc.nms(b, thr, order=order))
    ncls = 90
    cls = rng.randint(0, ncls, K).astype(np.int64)
    got = ops.batched_nms(T(b), T(sc), T(cls), thr).cpu().numpy()
    exp = np.concatenate([np.nonzero(cls == q)[0][orc.nms(b[cls == q], thr, order=np.argsort(-sc[cls == q], kind="stable"))] for q in range(ncls)])
    exp = exp[np.argsort(-sc[exp], kind="stable")]
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("regime", ["heavy", "sparse", "chain"])
def test_nms_cascade_regimes(ops, regime):
    """The cascade's three stages (K = 18 000 > NMS_CASCADE_MIN) under different survivor fractions: 'heavy' = piles of near-duplicates
    (almost everything dies in the filter), 'sparse' = almost nothing overlaps (everything survives into level 1), 'chain' = a long
    suppression chain that crosses the level boundary (box i overlaps box i + 1 only: kept / removed alternate, decided one from the other)."""
    rng = np.random.RandomState(9)
    K = 18000
    if regime == "heavy":
        centers = rng.rand(40, 2).astype(np.float32) * 0.6 + 0.2
        c = centers[rng.randint(0, 40, K)] + rng.randn(K, 2).astype(np.float32) * 0.004
        wh = np.float32(0.15) + rng.randn(K, 2).astype(np.float32) * 0.004
    elif regime == "sparse":
        c = rng.rand(K, 2).astype(np.float32) * 0.9 + 0.05
        wh = np.full((K, 2), 0.004, np.float32)
    else:
        t = np.arange(K, dtype=np.float32) / K
        c = np.stack([0.1 + 0.8 * t, np.full(K, 0.5, np.float32)], 1).astype(np.float32)
        wh = np.stack([np.full(K, 0.8 / K * 4, np.float32), np.full(K, 0.2, np.float32)], 1)       # IoU(i, i+1) = 3/5 > 0.5, IoU(i, i+2) = 1/3
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    thr = 0.5
    ko = orc.nms(b, thr)
    keep, _, cnt = ops.nms_sorted(T(b), thr)
    n = int(cnt.item())
    assert n == len(ko) and np.array_equal(keep[:n].cpu().numpy(), ko)
    cls = rng.randint(0, 7, K).astype(np.int64)                    # the class-aware instantiation through the same cascade
    sc = np.linspace(1.0, 0.0, K).astype(np.float32)
    got = ops.batched_nms(T(b), T(sc), T(cls), thr).cpu().numpy()
    exp = np.sort(np.concatenate([np.nonzero(cls == q)[0][orc.nms(b[cls == q], thr)] for q in range(7)]))
    assert np.array_equal(got, exp)


def test_nms_dense_clusters_near_threshold(ops):
    # many boxes piled on few objects with IoUs straddling the threshold: stresses the exact-division band
    rng = np.random.RandomState(3)
    K = 3000
    centers = rng.rand(12, 2).astype(np.float32) * 0.6 + 0.2
    cid = rng.randint(0, 12, K)
    c = centers[cid] + rng.randn(K, 2).astype(np.float32) * 0.01
    wh = np.float32(0.2) + rng.randn(K, 2).astype(np.float32) * 0.02
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    for thr in (0.7, 0.5, 0.3):
        keep_o = orc.nms(b, thr)
        keep, _, cnt = ops.nms_sorted(T(b), thr)
        assert int(cnt.item()) == len(keep_o) and np.array_equal(keep[:len(keep_o)].cpu().numpy(), keep_o)


def _with_nonfinite(rng, K):
    """Boxes as the reference can hand them to nms: SURVEY Q8 -- decode has no clamp on dw / dh, so exp overflows to inf, the centre
    arithmetic makes inf - inf = NaN, and clamp(0, 1) maps +-inf to 1 / 0 but leaves NaN in place (models/model.py:376-378 -> :394)."""
    c = rng.rand(K, 2).astype(np.float32) * 0.7 + 0.15
    wh = (rng.rand(K, 2).astype(np.float32) * 0.3 + 0.05)
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    bad = rng.choice(K, K // 9, replace=False)
    for n, i in enumerate(bad):
        kind = n % 6
        if kind == 0: b[i, rng.randint(0, 4)] = np.nan               # one NaN coordinate
        elif kind == 1: b[i] = np.nan                                # all NaN
        elif kind == 2: b[i, 2] = np.inf                             # infinite width: area inf, IoU 0 with everything finite
        elif kind == 3: b[i, 0], b[i, 2] = -np.inf, np.inf           # inf - (-inf) = inf
        elif kind == 4: b[i, 0], b[i, 2] = np.inf, np.inf            # inf - inf = NaN area
        else: b[i, 2:] = b[i, :2]                                    # zero area
    return b


@pytest.mark.parametrize("K,thr", [(5000, 0.7), (300, 0.3), (64, 0.5)])
def test_nms_nan_and_inf_boxes_follow_torchvision_semantics(ops, K, thr):
    """torchvision's nms (CPU and CUDA kernels alike) never tests for NaN: a box with a NaN coordinate has a NaN area, every IoU
    it takes part in is NaN, `NaN > thr` is false -- it is always KEPT and never suppresses anything; an infinite area gives
    inter / inf = 0.  The oracle restates exactly that expression; the HIP tiles decide without the division only when
    inter - thr (1 +- 2^-20) union is ordered, so every NaN pair falls through to the exact IEEE division (csrc/nms.hip)."""
    rng = np.random.RandomState(K)
    b = _with_nonfinite(rng, K)
    keep_o = orc.nms(b, thr)
    with np.errstate(invalid="ignore"):
        nanrow = np.isnan((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    assert nanrow.sum() > 0 and set(np.nonzero(nanrow)[0]) <= set(keep_o.tolist())      # NaN-area boxes are all kept
    keep, rois, cnt = ops.nms_sorted(T(b), thr, want_rois=True)
    n = int(cnt.item())
    assert n == len(keep_o) and np.array_equal(keep[:n].cpu().numpy(), keep_o)
    assert np.array_equal(rois[:n].cpu().numpy(), b[keep_o], equal_nan=True)
    # the drop-in entry points (sort by score first): scores finite, boxes not
    sc = rng.rand(K).astype(np.float32)
    order = np.argsort(-sc, kind="stable")
    assert np.array_equal(ops.nms(T(b), T(sc), thr).cpu().numpy(), orc.nms(b, thr, order=order))
    cls = rng.randint(0, 5, K).astype(np.int64)
    got = ops.batched_nms(T(b), T(sc), T(cls), thr).cpu().numpy()
    exp = np.concatenate([np.nonzero(cls == c)[0][orc.nms(b[cls == c], thr, order=np.argsort(-sc[cls == c], kind="stable"))] for c in range(5)])
    exp = exp[np.argsort(-sc[exp], kind="stable")]
    assert np.array_equal(got, exp)


def test_nms_in_kernel_handoff_under_uneven_load(ops):
    """nms_kernel hands the relation words from its tile waves to its resolver waves INSIDE one launch (write-through stores, a flag
    word per tile, sc1 polls + an agent acquire; csrc/nms.hip).  A stale word shows up as a different keep list, so: 150 launches
    with a changing amount of unrelated traffic on a second stream (uneven load, warm L2), every result compared with the oracle's.
    (With plain instead of write-through stores one launch in ~50 differs by a box on this input.)"""
    rng = np.random.RandomState(11)
    K = 12000
    c = np.stack([rng.rand(K) * 1000, rng.rand(K) * 600], 1).astype(np.float32)
    sz = np.array([128., 256., 512.], np.float32)[rng.randint(0, 3, K)] * np.exp(rng.randn(K) * 0.1).astype(np.float32)
    ar = np.array([0.5, 1., 2.], np.float32)[rng.randint(0, 3, K)]
    wh = np.stack([sz * np.sqrt(ar), sz / np.sqrt(ar)], 1).astype(np.float32)
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    b[:, 0::2] = b[:, 0::2].clip(0, 1000); b[:, 1::2] = b[:, 1::2].clip(0, 600)
    keep_o = orc.nms(b, 0.7)
    tb = T(b)
    side = torch.cuda.Stream()
    x = torch.randn(2048, 2048, device=DEV)
    bad = 0
    for it in range(150):
        with torch.cuda.stream(side):
            for _ in range(it % 5):
                x = torch.tanh(x @ x * 1e-3)
        keep, _, cnt = ops.nms_sorted(tb, 0.7)
        n = int(cnt.item())
        bad += int(n != len(keep_o) or not np.array_equal(keep[:n].cpu().numpy(), keep_o))
    torch.cuda.synchronize()
    assert bad == 0, "%d of 150 launches differ from the oracle" % bad


def test_in_kernel_handoffs_next_to_resident_foreign_workgroups(ops):
    """Multi-GPU readiness without the hardware: during training RCCL keeps persistent workgroups resident on the GPU while the hot
    path runs.  The launches with in-kernel hand-offs (tile -> resolver flags and the output ticket in nms_kernel, the grid barriers of
    rpn_match_kernel and topk_partition_kernel) assume their OWN workgroups become resident, not that the chip is empty: here 32, then
    96 foreign workgroups (frcnn_diag_occupy: a stand-in for RCCL's channels) sit on a side stream for the whole time, and every result
    must equal the oracle's -- proposals (top-k + NMS) and RPN targets with device sampling, at 600x1000."""
    from faster_rcnn_pytorch_amd import _lib
    from oracle import philox_ref
    rng = np.random.RandomState(17)
    H, W = 600, 1000
    anchor = orc.anchor_grid(H, W)
    N = anchor.shape[0]
    reg, cls = rpn_outputs(rng, N, "trained")
    rois_o, src_o = orc.region_proposal(reg, cls, anchor, 1 / 1000, 12000, 0.7, 2000)
    gt = _gt(rng, 6)
    pre, _, (n_pos, n_neg) = orc.rpn_targets(anchor, gt)
    pp = philox_ref.sampling_perm(5, 3, 1, np.nonzero(pre == 1)[0]); pn = philox_ref.sampling_perm(5, 3, 0, np.nonzero(pre == 0)[0])
    cls_o = orc.rpn_targets(anchor, gt, pp, pn)[0]
    treg, tcls, tanch, tgt = T(reg), T(cls), T(anchor), T(gt)
    side = torch.cuda.Stream()
    bad = 0
    for n_foreign in (32, 96):
        for it in range(25):
            _lib.diag_occupy(n_foreign, 400, side)                       # 400 us of residency: longer than the launches below take
            rois, cnt, src = ops.region_proposal(treg, tcls, tanch, 1 / 1000, 12000, 0.7, 2000, want_src=True)
            tc = ops.rpn_targets(tanch, tgt, seed=5, offset=3)[0]
            n = int(cnt.item())
            bad += int(n != len(rois_o) or not np.array_equal(src[:n].cpu().numpy(), src_o) or not np.array_equal(tc.cpu().numpy(), cls_o))
            side.synchronize()
    assert bad == 0, "%d of 50 iterations differ from the oracle" % bad


@pytest.mark.parametrize("env", ["FRCNN_TOPK_FUSED=0", "FRCNN_TOPK_FUSED=2", "FRCNN_NMS_FOLD_EMIT=0", "FRCNN_NMS_DENSE_MIN=1000", "FRCNN_RPN_FUSED=0"])
def test_alternative_launch_forms_give_the_same_results(env):
    """The library keeps the forms it measured against each other (three / two / one top-k launches, NMS outputs by nms_emit_kernel,
    the generic NMS relation layout below 16 384 boxes, the staged RPN target maker) behind environment switches that are read once
    per process: a child process per switch runs the proposal stage and the RPN target maker at 600x1000 and must reproduce the
    oracle's outputs exactly, like the default forms do in the tests above."""
    import os, subprocess, sys, tempfile
    from oracle import philox_ref
    rng = np.random.RandomState(23)
    anchor = orc.anchor_grid(600, 1000)
    N = anchor.shape[0]
    reg, cls = rpn_outputs(rng, N, "trained")
    rois_o, src_o = orc.region_proposal(reg, cls, anchor, 1 / 1000, 12000, 0.7, 2000)
    gt = _gt(rng, 5)
    pre, _, _ = orc.rpn_targets(anchor, gt)
    pp = philox_ref.sampling_perm(9, 4, 1, np.nonzero(pre == 1)[0]); pn = philox_ref.sampling_perm(9, 4, 0, np.nonzero(pre == 0)[0])
    cls_o = orc.rpn_targets(anchor, gt, pp, pn)[0]
    code = ("import numpy as np, torch, sys; from faster_rcnn_pytorch_amd import ops; d = sys.argv[1];"
            "L = lambda n: torch.from_numpy(np.load(d + '/' + n + '.npy')).cuda();"
            "rois, cnt, src = ops.region_proposal(L('reg'), L('cls'), L('anchor'), 1 / 1000, 12000, 0.7, 2000, want_src=True);"
            "n = int(cnt.item()); np.save(d + '/src.npy', src[:n].cpu().numpy()); np.save(d + '/rois.npy', rois[:n].cpu().numpy());"
            "np.save(d + '/tcls.npy', ops.rpn_targets(L('anchor'), L('gt'), seed=9, offset=4)[0].cpu().numpy())")
    with tempfile.TemporaryDirectory() as d:
        for n, a in (("reg", reg), ("cls", cls), ("anchor", anchor), ("gt", gt)):
            np.save(os.path.join(d, n + ".npy"), a)
        k, v = env.split("=")
        e = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        e[k] = v
        subprocess.run([sys.executable, "-c", code, d], check=True, env=e, timeout=300)
        assert np.array_equal(np.load(os.path.join(d, "src.npy")), src_o), env
        assert np.array_equal(np.load(os.path.join(d, "rois.npy")), rois_o), env
        assert np.array_equal(np.load(os.path.join(d, "tcls.npy")), cls_o), env


# ------------------------------------------------------------------------------------------ whole proposal stage
@pytest.mark.parametrize("regime,mode", [("init", "train"), ("trained", "train"), ("trained", "test")])
def test_region_proposal_full_size_bit_exact(ops, regime, mode):
    rng = np.random.RandomState(11)
    H, W = 600, 1000
    anchor = orc.anchor_grid(H, W)
    N = anchor.shape[0]
    reg, cls = rpn_outputs(rng, N, regime)
    K, P = (12000, 2000) if mode == "train" else (6000, 300)
    rois_o, src_o = orc.region_proposal(reg, cls, anchor, 1 / 1000, K, 0.7, P)
    # (a) anchors from HBM
    rois, cnt, src = ops.region_proposal(T(reg), T(cls), T(anchor), 1 / 1000, K, 0.7, P, want_src=True)
    n = int(cnt.item())
    assert n == len(rois_o)
    assert np.array_equal(src[:n].cpu().numpy(), src_o)          # integer indices: bit-exact
    assert np.array_equal(rois[:n].cpu().numpy(), rois_o)        # boxes: bit-exact (tolerance would be 1e-4)
    # (b) anchors regenerated in registers (never read from HBM)
    grid = (H // 16, W // 16, 16, ops.anchor_base(), W, H)
    rois2, cnt2, src2 = ops.region_proposal(T(reg), T(cls), None, 1 / 1000, K, 0.7, P, grid=grid, want_src=True)
    assert int(cnt2.item()) == n and torch.equal(src2[:n], src[:n]) and torch.equal(rois2[:n], rois[:n])


def test_region_proposal_properties_fpn_size(ops):
    # N = 268 569 is too slow for the O(N^2) oracle sort in CI; check size-independent properties instead
    rng = np.random.RandomState(5)
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    anchor = orc.tv_anchor_grid(800, 1344, shapes, normalise=True)
    N = anchor.shape[0]
    reg, cls = rpn_outputs(rng, N, "trained")
    rois, cnt, src = ops.region_proposal(T(reg), T(cls), T(anchor), 10 / 1000, 4000, 0.7, 1000, want_src=True)
    n = int(cnt.item())
    assert 0 < n <= 1000
    r = rois[:n].cpu().numpy()
    s = src[:n].cpu().numpy()
    assert len(np.unique(s)) == n
    b_o, s_o, _ = orc.proposal_prologue(reg, cls, anchor, 10 / 1000)
    assert np.array_equal(r, b_o[s])                              # rois are the decoded boxes of their anchors
    sc = s_o[s]
    assert (np.diff(sc) <= 0).all() and (sc >= 0).all()           # score-descending
    kth = np.sort(s_o)[::-1][3999]
    assert (sc >= kth).all()                                      # all from the top 4000
    iou = orc.pairwise_iou(r, r, 0.0)
    np.fill_diagonal(iou, 0)
    assert iou.max() <= 0.7                                       # survivors do not suppress each other
    assert list(orc.nms(r, 0.7)) == list(range(n))                # idempotence


# ------------------------------------------------------------------------------------------ target makers
def _gt(rng, G):
    c = rng.rand(G, 2) * 0.7 + 0.15
    wh = rng.rand(G, 2) * 0.52 + 0.08
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


@pytest.mark.parametrize("variant,G,seed", [(0, 1, 0), (0, 3, 1), (0, 8, 2), (1, 5, 3), (0, 40, 4)])
def test_rpn_targets_host_perm_parity(ops, variant, G, seed):
    rng = np.random.RandomState(seed)
    if variant == 0:
        anchor = orc.anchor_grid(600, 1000)
    else:
        anchor = orc.tv_anchor_grid(320, 480, [(80, 120), (40, 60), (20, 30), (10, 15), (5, 8)], normalise=True)
    gt = _gt(rng, G)
    _, _, (n_pos, n_neg) = orc.rpn_targets(anchor, gt, variant=variant)
    cls, reg, counts = ops.rpn_targets(T(anchor), T(gt), variant=variant)        # first call: learn the counts
    assert counts[:2].cpu().tolist() == [n_pos, n_neg]
    # the reference draws randperm(n_pos) only if n_pos > 128, randperm(n_neg) only if n_neg > 256 - n_pos
    g = torch.Generator().manual_seed(seed)
    pp = torch.randperm(n_pos, generator=g).numpy() if n_pos > 128 else None
    pn = torch.randperm(n_neg, generator=g).numpy() if n_neg > 256 - n_pos else None
    cls_o, reg_o, _ = orc.rpn_targets(anchor, gt, pp, pn, variant=variant)
    cls, reg, counts = ops.rpn_targets(T(anchor), T(gt), variant=variant, perm_pos=pp, perm_neg=pn)
    assert counts.cpu().tolist()[2] == 0
    assert np.array_equal(cls.cpu().numpy(), cls_o)                               # labels: bit-exact
    r = reg.cpu().numpy()
    assert np.array_equal(r[:, :2], reg_o[:, :2])
    assert np.abs(r[:, 2:] - reg_o[:, 2:]).max() < 1e-6                           # logf tolerance 1e-6
    npe = min(n_pos, 128)
    assert (cls_o == 1).sum() == npe and (cls_o == 0).sum() == min(n_neg, 256 - npe)


def test_rpn_targets_many_positives_forces_pos_sampling(ops):
    # a gt equal to a large anchor region -> hundreds of IoU >= 0.7 anchors? use many gts to exceed 128 positives
    rng = np.random.RandomState(9)
    anchor = orc.anchor_grid(600, 1000)
    ins = (anchor[:, 0] >= 0) & (anchor[:, 1] >= 0) & (anchor[:, 2] <= 1) & (anchor[:, 3] <= 1)
    gt = anchor[ins][rng.choice(ins.sum(), 200, replace=False)]                    # 200 gts == anchors -> >= 200 positives
    _, _, (n_pos, n_neg) = orc.rpn_targets(anchor, gt)
    assert n_pos > 128
    g = torch.Generator().manual_seed(0)
    pp = torch.randperm(n_pos, generator=g).numpy()
    pn = torch.randperm(n_neg, generator=g).numpy()
    cls_o, _, _ = orc.rpn_targets(anchor, gt, pp, pn)
    cls, _, counts = ops.rpn_targets(T(anchor), T(gt), perm_pos=pp, perm_neg=pn)
    assert counts.cpu().tolist()[:3] == [n_pos, n_neg, 0]
    assert np.array_equal(cls.cpu().numpy(), cls_o)
    assert (cls_o == 1).sum() == 128 and (cls_o == 0).sum() == 128


def test_rpn_targets_device_sampling_properties(ops):
    rng = np.random.RandomState(4)
    anchor = orc.anchor_grid(600, 1000)
    gt = _gt(rng, 6)
    pre, _, (n_pos, n_neg) = orc.rpn_targets(anchor, gt)
    a = ops.rpn_targets(T(anchor), T(gt), seed=123, offset=0)[0].cpu().numpy()
    b = ops.rpn_targets(T(anchor), T(gt), seed=123, offset=0)[0].cpu().numpy()
    c = ops.rpn_targets(T(anchor), T(gt), seed=124, offset=0)[0].cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, c)      # deterministic in (seed, offset)
    npe = min(n_pos, 128)
    assert (a == 1).sum() == npe and (a == 0).sum() == min(n_neg, 256 - npe)
    assert ((a == 1) <= (pre == 1)).all() and ((a == 0) <= (pre == 0)).all()   # sampling only demotes to -1
    # uniformity smoke check: kept negatives spread over the whole candidate list
    kept = np.nonzero(a == 0)[0]
    cand = np.nonzero(pre == 0)[0]
    q = np.searchsorted(cand, kept) / len(cand)
    assert 0.35 < q.mean() < 0.65


def test_rpn_targets_device_sampling_fpn_size_equals_reference_with_philox_permutations(ops):
    """N = 268 569 (config F) takes rpn_match + rpn_apply; with only the negatives over quota (G = 8) and with both classes over quota
    (G = 300) it must pick exactly what the oracle picks when it is fed the Philox permutations (oracle/philox_ref.py)."""
    from oracle import philox_ref
    rng = np.random.RandomState(12)
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    anchor = orc.tv_anchor_grid(800, 1344, shapes, normalise=True)
    ins = np.nonzero((anchor[:, 0] >= 0) & (anchor[:, 1] >= 0) & (anchor[:, 2] <= 1) & (anchor[:, 3] <= 1))[0]
    for G, tag in ((8, "neg-only"), (300, "pos+neg")):
        gt = anchor[ins[rng.choice(len(ins), G, replace=False)]] if G > 100 else _gt(rng, G)
        pre, _, (n_pos, n_neg) = orc.rpn_targets(anchor, gt, variant=1)
        if G > 100:
            assert n_pos > 128
        a = ops.rpn_targets(T(anchor), T(gt), variant=1, seed=77, offset=5)[0].cpu().numpy()
        npe = min(n_pos, 128)
        assert (a == 1).sum() == npe and (a == 0).sum() == min(n_neg, 256 - npe), tag
        assert ((a == 1) <= (pre == 1)).all() and ((a == 0) <= (pre == 0)).all()
        pp = philox_ref.sampling_perm(77, 5, 1, np.nonzero(pre == 1)[0]); pn = philox_ref.sampling_perm(77, 5, 0, np.nonzero(pre == 0)[0])
        assert np.array_equal(a, orc.rpn_targets(anchor, gt, pp, pn, variant=1)[0]), tag


def test_philox_state_on_device_equals_by_value_and_advances(ops):
    """ABI v4: the target makers can take (seed, offset) from a device-resident int64[2]; a call uses the pair it finds and leaves
    offset + 1 behind.  Same samples as the by-value form for the same (seed, offset); consecutive calls walk the offsets."""
    rng = np.random.RandomState(21)
    gt = _gt(rng, 6)
    lab = rng.randint(0, 20, 6).astype(np.int64)
    seed = 0x9E3779B97F4A7C15                                   # exercises the high half and the sign bit of the int64 carrier
    st = ops.philox_state(seed, 40, DEV)
    rois = rand_boxes(rng, 2000, 0.05, 0.5)
    rois[:100] = np.clip(gt[rng.randint(0, 6, 100)] + rng.randn(100, 4).astype(np.float32) * 0.01, 0, 1)
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    cases = [(orc.anchor_grid(600, 1000), 0), (orc.tv_anchor_grid(800, 1344, shapes, normalise=True), 1)]   # single-workgroup / chip-wide sampler
    off = 40
    for anchor, variant in cases:
        for _ in range(2):
            a = ops.rpn_targets(T(anchor), T(gt), variant=variant, philox_state=st)[0]
            b = ops.rpn_targets(T(anchor), T(gt), variant=variant, seed=seed, offset=off)[0]
            assert torch.equal(a, b)
            off += 1
            assert st.cpu().tolist()[1] == off
    k1 = ops.head_targets(T(rois), T(gt), T(lab), philox_state=st, want_keep=True)[3]
    k2 = ops.head_targets(T(rois), T(gt), T(lab), seed=seed, offset=off, want_keep=True)[3]
    k3 = ops.head_targets(T(rois), T(gt), T(lab), philox_state=st, want_keep=True)[3]
    assert torch.equal(k1, k2) and not torch.equal(k1, k3)
    assert st.cpu().tolist()[1] == off + 2
    assert (st.cpu().tolist()[0] & ((1 << 64) - 1)) == seed


def test_region_proposal_per_level_nms_option(ops):
    """Optional per-FPN-level NMS (BASELINE configs[3] wording; the reference itself runs ONE global NMS, new_model.py:74-83):
    same global top-K, then boxes compete only inside their level.  Oracle = a per-level loop over orc.nms."""
    rng = np.random.RandomState(8)
    shapes = [(48, 64), (24, 32), (12, 16), (6, 8), (3, 4)]
    H, W = 192, 256
    anchor = orc.tv_anchor_grid(H, W, shapes, normalise=True)
    N = anchor.shape[0]
    offs = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in shapes])])
    assert offs[-1] == N
    reg, cls = rpn_outputs(rng, N, "trained")
    reg *= 0.3                                                   # keep neighbours overlapping across levels too
    K, P = 3000, 500
    b_o, s_o, _ = orc.proposal_prologue(reg, cls, anchor, 10 / 1000)
    idx, _ = orc.topk_sorted(s_o, K)
    sb = b_o[idx]
    lvl = np.searchsorted(offs, idx, side="right") - 1
    kept = np.sort(np.concatenate([np.nonzero(lvl == l)[0][orc.nms(sb[lvl == l], 0.7)] for l in range(5)]))[:P]
    glob = orc.nms(sb, 0.7)[:P]
    assert not np.array_equal(kept, glob[:len(kept)])            # the option must matter on this input
    rois, cnt, src = ops.region_proposal(T(reg), T(cls), T(anchor), 10 / 1000, K, 0.7, P, want_src=True, nms_level_offsets=offs)
    n = int(cnt.item())
    assert n == len(kept) and np.array_equal(src[:n].cpu().numpy(), idx[kept]) and np.array_equal(rois[:n].cpu().numpy(), sb[kept])
    rois, cnt, src = ops.region_proposal(T(reg), T(cls), T(anchor), 10 / 1000, K, 0.7, P, want_src=True)      # default: global
    n = int(cnt.item())
    assert n == len(glob) and np.array_equal(src[:n].cpu().numpy(), idx[glob])
    with pytest.raises(ValueError):
        ops.region_proposal(T(reg), T(cls), T(anchor), 10 / 1000, K, 0.7, P, nms_level_offsets=[0, 5, 3, N])


@pytest.mark.parametrize("variant,label_offset,max_pos,total,P", [(0, 1, 32, 128, 2000), (0, 1, 32, 128, 300), (1, 0, 128, 512, 1000)])
def test_head_targets_host_perm_parity(ops, variant, label_offset, max_pos, total, P):
    rng = np.random.RandomState(P + variant)
    G = 5
    gt = _gt(rng, G)
    lab = rng.randint(0, 20, G).astype(np.int64) + (1 - label_offset)
    rois = rand_boxes(rng, P, 0.05, 0.5)
    rois[:40] = np.clip(gt[rng.randint(0, G, 40)] + rng.randn(40, 4).astype(np.float32) * 0.01, 0, 1)
    n_live = P - 13
    npc, nnc = orc.head_target_counts(rois[:n_live], gt, lab, variant)
    g = torch.Generator().manual_seed(1)
    pp = torch.randperm(npc, generator=g).numpy()                 # the reference always draws both (model_.py:149,155)
    pn = torch.randperm(nnc, generator=g).numpy()
    cls_o, reg_o, rois_o, keep_o = orc.head_targets(rois[:n_live], gt, lab, pp, pn, variant, label_offset, max_pos, total)
    cls, reg, srois, keep, counts = ops.head_targets(T(rois), T(gt), T(lab), n_rois=T(np.array([n_live], np.int32)), variant=variant,
                                                     label_offset=label_offset, max_pos=max_pos, total=total, perm_pos=pp, perm_neg=pn,
                                                     want_keep=True)
    assert counts.cpu().tolist() == [npc, nnc, len(cls_o), 0]
    assert len(cls_o) == total
    assert np.array_equal(keep.cpu().numpy(), keep_o) and np.array_equal(cls.cpu().numpy(), cls_o)
    assert np.array_equal(srois.cpu().numpy(), rois_o)
    assert np.allclose(reg.cpu().numpy(), reg_o, rtol=0, atol=1e-5)               # logf then /0.2: tolerance 1e-5


@pytest.mark.parametrize("size", ["vgg-inline", "fpn-two-launches"])
def test_rpn_targets_device_sampling_equals_reference_with_philox_permutations(ops, size):
    """Device-RNG mode = the reference's randperm sampling (models/model.py:225-236) run with perm = argsort of the Philox keys
    (oracle/philox_ref.py, pinned by the Random123 vectors): the oracle's host-permutation path, fed those permutations, gives the
    EXACT expected labels -- for the one-launch form (N <= 24 576) and the rpn_match + rpn_apply form, with and without a
    subsampled positive class."""
    from oracle import philox_ref
    rng = np.random.RandomState(21)
    if size == "vgg-inline":
        anchor, variant = orc.anchor_grid(600, 1000), 0
    else:
        anchor, variant = orc.tv_anchor_grid(800, 1344, [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)], normalise=True), 1
    ins = np.nonzero((anchor[:, 0] >= 0) & (anchor[:, 1] >= 0) & (anchor[:, 2] <= 1) & (anchor[:, 3] <= 1))[0]
    for G, seed, offset in ((5, 11, 0), (1, (5 << 32) | 9, (1 << 32) | 7), (200, 3, 12345)):
        gt = anchor[ins[rng.choice(len(ins), G, replace=False)]] if G > 100 else _gt(rng, G)
        pre, _, (n_pos, n_neg) = orc.rpn_targets(anchor, gt, variant=variant)
        pp = philox_ref.sampling_perm(seed, offset, 1, np.nonzero(pre == 1)[0])
        pn = philox_ref.sampling_perm(seed, offset, 0, np.nonzero(pre == 0)[0])
        cls_o, reg_o, _ = orc.rpn_targets(anchor, gt, pp, pn, variant=variant)
        cls, reg, counts = ops.rpn_targets(T(anchor), T(gt), variant=variant, seed=seed, offset=offset)
        assert counts.cpu().tolist()[:3] == [n_pos, n_neg, 0]
        assert np.array_equal(cls.cpu().numpy(), cls_o), (size, G)                  # labels AFTER sampling: bit-exact
        r = reg.cpu().numpy()
        assert np.array_equal(r[:, :2], reg_o[:, :2]) and np.abs(r[:, 2:] - reg_o[:, 2:]).max() < 1e-6   # logf tolerance, as in the host-perm test
        if G > 100:
            assert n_pos > 128                                       # the positive class was subsampled too


def test_rpn_targets_staged_chipwide_sampler_equals_reference_with_philox_permutations():
    """The staged form at FPN size (rpn_colmax -> rpn_label with keys and key histogram -> rpn_apply: what the launcher falls back to when
    the fused grid could not be co-resident) draws the same Philox keys: a child process with FRCNN_RPN_FUSED=0 must reproduce the labels
    the oracle gives for the Philox permutations, with a subsampled positive class."""
    import os, subprocess, sys, tempfile
    from oracle import philox_ref
    rng = np.random.RandomState(33)
    anchor = orc.tv_anchor_grid(800, 1344, [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)], normalise=True)
    ins = np.nonzero((anchor[:, 0] >= 0) & (anchor[:, 1] >= 0) & (anchor[:, 2] <= 1) & (anchor[:, 3] <= 1))[0]
    gt = anchor[ins[rng.choice(len(ins), 180, replace=False)]]
    pre, _, (n_pos, n_neg) = orc.rpn_targets(anchor, gt, variant=1)
    assert n_pos > 128
    pp = philox_ref.sampling_perm(21, 6, 1, np.nonzero(pre == 1)[0]); pn = philox_ref.sampling_perm(21, 6, 0, np.nonzero(pre == 0)[0])
    cls_o = orc.rpn_targets(anchor, gt, pp, pn, variant=1)[0]
    code = ("import numpy as np, torch, sys; from faster_rcnn_pytorch_amd import ops; d = sys.argv[1];"
            "a = torch.from_numpy(np.load(d + '/anchor.npy')).cuda(); g = torch.from_numpy(np.load(d + '/gt.npy')).cuda();"
            "np.save(d + '/out.npy', ops.rpn_targets(a, g, variant=1, seed=21, offset=6)[0].cpu().numpy())")
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "anchor.npy"), anchor), np.save(os.path.join(d, "gt.npy"), gt)
        env = dict(os.environ, FRCNN_RPN_FUSED="0", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        subprocess.run([sys.executable, "-c", code, d], check=True, env=env, timeout=300)
        assert np.array_equal(np.load(os.path.join(d, "out.npy")), cls_o)


def test_rpn_targets_staged_device_rng_small_shape_equals_reference_and_leaves_workspace_zero():
    """The staged device-RNG form (FRCNN_RPN_FUSED=0: rpn_colmax -> rpn_label with keys -> rpn_apply) at N = 3285, a ragged tail for its
    256- and 1024-thread blocks: (a) both classes over quota, (b) only the negatives.  One child process makes three calls per case:
    (seed, offset) by value = the oracle with the Philox permutations; from a device philox_state = the same labels, offset + 1 left
    behind (the snapshot hand-off between the launches); by value again = the first call (the shared sampler workspace was left zero)."""
    import os, subprocess, sys, tempfile
    from oracle import philox_ref
    anchor = orc.tv_anchor_grid(96, 136, [(24, 34), (12, 17), (6, 9), (3, 5), (2, 3)], normalise=True)
    assert anchor.shape[0] == 3285
    l0 = anchor[:24 * 34 * 3]
    ins = np.nonzero((l0[:, 0] >= 0) & (l0[:, 1] >= 0) & (l0[:, 2] <= 1) & (l0[:, 3] <= 1))[0]
    rng = np.random.RandomState(1)
    gts = [l0[ins[rng.choice(len(ins), 140, replace=False)]], _gt(rng, 3)]          # oracle: (n_pos, n_neg) = (559, 1088) and (8, 2853)
    seed, offset = 31, 9
    code = ("import numpy as np, torch, sys; from faster_rcnn_pytorch_amd import ops; d = sys.argv[1];"
            "L = lambda n: torch.from_numpy(np.load(d + '/' + n + '.npy')).cuda(); a = L('anchor')\n"
            "for c in '01':\n"
            "    g = L('gt' + c); st = ops.philox_state(%d, %d, 'cuda')\n"
            "    r = [ops.rpn_targets(a, g, variant=1, seed=%d, offset=%d), ops.rpn_targets(a, g, variant=1, philox_state=st),"
            " ops.rpn_targets(a, g, variant=1, seed=%d, offset=%d)]\n"
            "    np.save(d + '/cls' + c + '.npy', np.stack([x[0].cpu().numpy() for x in r]))\n"
            "    np.save(d + '/counts' + c + '.npy', np.stack([x[2].cpu().numpy() for x in r])); np.save(d + '/st' + c + '.npy', st.cpu().numpy())\n"
            % (seed, offset, seed, offset, seed, offset))
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "anchor.npy"), anchor), np.save(os.path.join(d, "gt0.npy"), gts[0]), np.save(os.path.join(d, "gt1.npy"), gts[1])
        env = dict(os.environ, FRCNN_RPN_FUSED="0", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        subprocess.run([sys.executable, "-c", code, d], check=True, env=env, timeout=300)
        for c, gt in enumerate(gts):
            pre, _, (n_pos, n_neg) = orc.rpn_targets(anchor, gt, variant=1)
            assert n_neg > 256 - min(n_pos, 128) and (n_pos > 128) == (c == 0), (c, n_pos, n_neg)   # the classes meant to be subsampled are
            pp = philox_ref.sampling_perm(seed, offset, 1, np.nonzero(pre == 1)[0]); pn = philox_ref.sampling_perm(seed, offset, 0, np.nonzero(pre == 0)[0])
            cls_o = orc.rpn_targets(anchor, gt, pp, pn, variant=1)[0]
            cls, counts = np.load(os.path.join(d, "cls%d.npy" % c)), np.load(os.path.join(d, "counts%d.npy" % c))
            for k in range(3):
                assert np.array_equal(cls[k], cls_o), (c, k)
                assert counts[k, :3].tolist() == [n_pos, n_neg, 0], (c, k)
            assert np.load(os.path.join(d, "st%d.npy" % c)).tolist() == [seed, offset + 1]


@pytest.mark.parametrize("variant,label_offset,max_pos,total,P", [(0, 1, 32, 128, 2000), (1, 0, 128, 512, 1000), (0, 1, 32, 128, 300)])
def test_head_targets_device_sampling_equals_reference_with_philox_permutations(ops, variant, label_offset, max_pos, total, P):
    """FastRcnnTargetMaker in device-RNG mode = the reference (models/model.py:318-345) with perm = argsort of the Philox keys of the
    candidate lists (streams 2 = positives, 3 = negatives; element = candidate index into [rois; gt]): rows, classes, targets and
    sampled RoIs bit-exact against the oracle's host-permutation path."""
    from oracle import philox_ref
    rng = np.random.RandomState(31 + P)
    G = 6
    gt = _gt(rng, G)
    lab = rng.randint(0, 20, G).astype(np.int64)
    rois = rand_boxes(rng, P, 0.05, 0.5)
    n_near = P // 5                                                  # enough positives to subsample them as well
    rois[:n_near] = np.clip(gt[rng.randint(0, G, n_near)] + rng.randn(n_near, 4).astype(np.float32) * 0.02, 0, 1)
    npc, nnc = orc.head_target_counts(rois, gt, lab, variant=variant)
    for seed, offset in ((5, 0), ((2 << 32) | 1, 99)):
        keep_dev = ops.head_targets(T(rois), T(gt), T(lab), variant=variant, label_offset=label_offset, max_pos=max_pos, total=total,
                                    seed=seed, offset=offset, want_keep=True)
        # the candidate lists: identity permutations make the oracle return them in list order
        full = orc.head_targets(rois, gt, lab, np.arange(npc), np.arange(nnc), variant=variant, label_offset=label_offset, max_pos=npc, total=npc + nnc)
        pos_list, neg_list = full[3][:npc], full[3][npc:]
        pp = philox_ref.sampling_perm(seed, offset, 2, pos_list)
        pn = philox_ref.sampling_perm(seed, offset, 3, neg_list)
        cls_o, reg_o, rois_o, keep_o = orc.head_targets(rois, gt, lab, pp, pn, variant=variant, label_offset=label_offset, max_pos=max_pos, total=total)
        assert keep_dev[4].cpu().tolist()[:2] == [npc, nnc]
        assert np.array_equal(keep_dev[3].cpu().numpy()[:len(keep_o)], keep_o)
        assert np.array_equal(keep_dev[0].cpu().numpy()[:len(cls_o)], cls_o)
        assert np.array_equal(keep_dev[2].cpu().numpy()[:len(rois_o)], rois_o)
        assert np.allclose(keep_dev[1].cpu().numpy()[:len(reg_o)], reg_o, atol=1e-6)


def test_head_targets_device_sampling_properties(ops):
    rng = np.random.RandomState(2)
    G, P = 4, 2000
    gt = _gt(rng, G)
    lab = rng.randint(0, 20, G).astype(np.int64)
    rois = rand_boxes(rng, P, 0.05, 0.5)
    rois[:100] = np.clip(gt[rng.randint(0, G, 100)] + rng.randn(100, 4).astype(np.float32) * 0.01, 0, 1)
    npc, nnc = orc.head_target_counts(rois, gt, lab)
    out1 = ops.head_targets(T(rois), T(gt), T(lab), seed=5, want_keep=True)
    out2 = ops.head_targets(T(rois), T(gt), T(lab), seed=5, want_keep=True)
    out3 = ops.head_targets(T(rois), T(gt), T(lab), seed=6, want_keep=True)
    keep = out1[3].cpu().numpy()
    assert np.array_equal(keep, out2[3].cpu().numpy()) and not np.array_equal(keep, out3[3].cpu().numpy())
    assert out1[4].cpu().tolist() == [npc, nnc, 128, 0]
    n_pos = min(npc, 32)
    allr = np.concatenate([rois, gt])
    iou = orc.pairwise_iou(allr, gt, 1e-5)
    mx, am = iou.max(1), iou.argmax(1)
    assert len(np.unique(keep)) == 128
    assert (mx[keep[:n_pos]] >= 0.5).all() and (mx[keep[n_pos:]] < 0.5).all()
    cls = out1[0].cpu().numpy()
    assert np.array_equal(cls[:n_pos], lab[am[keep[:n_pos]]] + 1) and (cls[n_pos:] == 0).all()
    assert np.array_equal(out1[2].cpu().numpy(), allr[keep])
    e = orc.encode(orc.xy_to_cxcy(gt[am[keep]]), orc.xy_to_cxcy(allr[keep])) / np.array([0.1, 0.1, 0.2, 0.2], np.float32)
    assert np.allclose(out1[1].cpu().numpy(), e, atol=1e-5)


# ------------------------------------------------------------------------------------------ RoIPool
def test_roi_pool_known_answers(ops):
    f = np.arange(16, dtype=np.float32).reshape(1, 1, 4, 4)
    out = ops.roi_pool(T(f), T(np.array([[0, 0, 3, 3]], np.float32)), (2, 2), 1.0)
    assert out.reshape(-1).cpu().tolist() == [5, 7, 13, 15]
    out = ops.roi_pool(T(f), T(np.array([[0.5, 0.5, 2.5, 2.5]], np.float32)), (1, 1), 1.0)   # round half away from zero
    assert out.item() == 15
    out = ops.roi_pool(T(f), T(np.array([[10, 10, 12, 12]], np.float32)), (2, 2), 1.0)       # outside -> empty bins -> 0
    assert (out == 0).all()


@pytest.mark.parametrize("C,H,W,R", [(512, 37, 62, 128), (512, 37, 62, 300), (3, 9, 11, 5), (64, 50, 50, 17)])
def test_roi_pool_fwd_bwd_vs_oracle(ops, C, H, W, R):
    rng = np.random.RandomState(C + R)
    f = rng.randn(C, H, W).astype(np.float32)
    rois = rand_boxes(rng, R, 0.02, 0.9) * np.array([W, H, W, H], np.float32)     # reference pre-scales by (fw,fh)
    rois[0] = [0, 0, W, H]
    rois[1] = [W * 0.5, H * 0.5, W * 0.5, H * 0.5]
    out_o, arg_o = orc.roi_pool_fwd(f, rois, 7, 7, 1.0)
    ft = T(f[None]).requires_grad_(True)
    out = ops.RoIPool((7, 7), 1.0)(ft, [T(rois)])
    assert np.array_equal(out.detach().cpu().numpy(), out_o)                      # max-pool values: bit-exact
    go = rng.randn(*out_o.shape).astype(np.float32)
    out.backward(T(go))
    gf_o = orc.roi_pool_bwd(go, arg_o, C, H, W)
    assert np.allclose(ft.grad[0].cpu().numpy(), gf_o, rtol=1e-5, atol=1e-5)      # fp32 sum order differs: 1e-5


def test_roi_pool_backward_duplicate_maxima_and_bit_reproducible(ops):
    """The round-5 backward (csrc/roi_pool.hip: wave-private planes, plain read-modify-write adds ranked among a bin's four lower
    neighbours; ds_add_f32 only for RoIs under 7 x 7 cells) at the training shape, on inputs that maximise what it must get right:
    a PIECEWISE-CONSTANT feature map (every bin of a flat patch takes the first pixel of its window, so neighbouring bins -- whose windows
    overlap by a row / column -- share their maximum all over the place, in 2 x 2 groups too), RoIs of every size (tiny ones: many bins on
    one pixel; sides of exactly 7 and 8 cells: bin sides 1 and 8/7), empty bins.  Gradient vs the oracle (1e-5: another fp32 order),
    bit-identical over repeated launches, and equal to the int32-ABI backward (which is given no boxes and adds with ds_add_f32)."""
    rng = np.random.RandomState(5)
    C, H, W, R = 512, 37, 62, 128
    f = np.repeat(np.repeat(rng.randn(C, 10, 16).astype(np.float32), 4, axis=1), 4, axis=2)[:, :H, :W].copy()      # 4 x 4 flat patches
    f[::3] += (rng.randn(C // 3 + 1, H, W) * 0.01).astype(np.float32)[:len(f[::3])]                               # a third of the channels: near-ties instead
    wh = rng.rand(R, 2) * np.array([0.9, 0.9]) + 0.02
    c = rng.rand(R, 2)
    rois = (np.concatenate([c - wh / 2, c + wh / 2], 1).clip(0, 1) * np.array([W, H, W, H])).astype(np.float32)
    rois[0] = [3, 2, 9, 8]            # 7 x 7 cells: bin sides exactly 1
    rois[1] = [3, 2, 10, 9]           # 8 x 8 cells: bin sides 8/7
    rois[2] = [5, 5, 6, 6]            # 2 x 2 cells: most bins share a pixel
    rois[3] = [20, 10, 26, 30]        # 7 wide, 21 tall
    rois[4] = [W + 2, H + 2, W + 5, H + 5]   # outside: empty bins
    rois[5] = [0, 0, W, H]
    out_o, arg_o = orc.roi_pool_fwd(f, rois, 7, 7, 1.0)
    go = rng.randn(*out_o.shape).astype(np.float32)
    ref = orc.roi_pool_bwd(go, arg_o, C, H, W)
    grads = []
    for _ in range(4):
        ft = T(f[None]).requires_grad_(True)
        out = ops.roi_pool(ft, T(rois), (7, 7), 1.0)
        assert np.array_equal(out.detach().cpu().numpy(), out_o)
        out.backward(T(go))
        grads.append(ft.grad[0].cpu().numpy())
    # how much of the input is the hard case: elements that share their pixel with another bin of the same (RoI, channel)
    a = arg_o.reshape(R, C, 49)
    dup = sum(int((np.sort(a[r], axis=1)[:, 1:] == np.sort(a[r], axis=1)[:, :-1])[np.sort(a[r], axis=1)[:, 1:] >= 0].sum()) for r in range(R))
    assert dup > 0.1 * a.size
    assert np.allclose(grads[0], ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    for g in grads[1:]:
        assert np.array_equal(g, grads[0])                                          # one summation order: bit-reproducible
    # the torchvision-shaped pair on the same inputs (int32 argmax, no boxes in backward)
    from faster_rcnn_pytorch_amd import _lib
    out32, arg32 = ops.roi_pool_with_argmax(T(f[None]), T(rois), (7, 7), 1.0)
    gf = torch.empty((1, C, H, W), dtype=torch.float32, device=DEV)
    got = T(go)
    _lib.check(_lib.lib.frcnn_roi_pool_bwd(got.data_ptr(), arg32.data_ptr(), R, C, H, W, 7, 7, gf.data_ptr(), torch.cuda.current_stream().cuda_stream), "roi_pool_bwd")
    torch.cuda.synchronize()
    assert np.allclose(gf[0].cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def test_roi_pool_backward_large_bin_grid(ops):
    """17 x 17 bins: one channel-pair run (2 * 289 elements) is longer than the LDS backward kernel's 512-thread pass; the generic int32
    entry point must route such shapes to the one-channel kernel instead of writing an all-zero gradient."""
    rng = np.random.RandomState(17)
    C, H, W, R, PH = 6, 40, 50, 9, 17
    feat = rng.randn(C, H, W).astype(np.float32)
    rois = rand_boxes(rng, R, 0.2, 0.9) * np.array([W, H, W, H], np.float32)
    out_o, arg_o = orc.roi_pool_fwd(feat, rois, PH, PH, 1.0)
    out, arg = ops.roi_pool_with_argmax(T(feat[None]), T(rois), (PH, PH), 1.0)
    assert np.array_equal(out.cpu().numpy(), out_o) and np.array_equal(arg.cpu().numpy(), arg_o)
    ft = T(feat[None]).requires_grad_(True)
    o = ops.roi_pool(ft, T(rois), (PH, PH), 1.0)
    go = rng.randn(*out_o.shape).astype(np.float32)
    o.backward(T(go))
    ref = orc.roi_pool_bwd(go, arg_o, C, H, W)
    assert np.abs(ref).sum() > 0 and np.allclose(ft.grad[0].cpu().numpy(), ref, atol=1e-5)


@pytest.mark.parametrize("C,H,W,R", [(512, 37, 62, 128), (6, 9, 11, 5), (3, 70, 70, 9)])
def test_roi_pool_int32_argmax_abi_bit_exact(ops, C, H, W, R):
    """The torchvision-shaped entry points (int32 argmax, -1 = empty bin): values AND argmax bit-exact, backward from them."""
    rng = np.random.RandomState(C * 7 + R)
    f = rng.randn(C, H, W).astype(np.float32)
    rois = rand_boxes(rng, R, 0.02, 0.9) * np.array([W, H, W, H], np.float32)
    rois[0] = [W + 3, H + 3, W + 9, H + 9]                                          # outside: empty bins, argmax -1
    out_o, arg_o = orc.roi_pool_fwd(f, rois, 7, 7, 1.0)
    out, arg = ops.roi_pool_with_argmax(T(f[None]), T(rois), (7, 7), 1.0)
    assert np.array_equal(out.cpu().numpy(), out_o) and np.array_equal(arg.cpu().numpy(), arg_o)
    assert (arg_o[0] == -1).all()


# ------------------------------------------------------------------------------------------ RoIAlign
def test_level_map_bit_exact(ops):
    rng = np.random.RandomState(0)
    rois = rand_boxes(rng, 5000, 0.005, 0.95) * np.array([1344, 800, 1344, 800], np.float32)
    sq = np.array([[0, 0, s, s] for s in (50, 111.9, 112, 223.9, 224, 447.9, 448, 895, 896, 2000, 0)], np.float32)
    rois = np.concatenate([sq, rois])
    assert np.array_equal(ops.roi_level_map(T(rois)).cpu().numpy(), orc.roi_level_map(rois))


def test_ms_roi_align_fwd_bwd_vs_oracle(ops):
    rng = np.random.RandomState(1)
    C = 16
    shapes = [(100, 168), (50, 84), (25, 42), (13, 21)]
    feats = [rng.randn(C, h, w).astype(np.float32) for h, w in shapes]
    rois = rand_boxes(rng, 60, 0.02, 0.9) * np.array([672, 400, 672, 400], np.float32)
    rois[0] = [-20, -10, 100, 90]
    rois[1] = [600, 350, 700, 420]
    out_o, lv = orc.ms_roi_align(feats, rois)
    assert len(set(lv.tolist())) >= 3
    fts = [T(f[None]).requires_grad_(True) for f in feats]
    m = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    out = m({str(i): f for i, f in enumerate(fts)}, [T(rois)], [(672, 400)])
    assert np.abs(out.detach().cpu().numpy() - out_o).max() < 1e-5               # tolerance 1e-5 (north star 1e-4)
    go = rng.randn(*out_o.shape).astype(np.float32)
    out.backward(T(go))
    for l, f in enumerate(fts):
        gf_o = orc.roi_align_bwd(go, feats[l].shape, rois, 0.25 / (1 << l), 2, False, lv, l)
        assert np.allclose(f.grad[0].cpu().numpy(), gf_o, rtol=1e-4, atol=1e-4)  # another (fixed) fp32 order than the oracle's scatter; bit for bit: test_gpu_roi_align_exact.py


@pytest.mark.parametrize("regime", ["proposal_like", "spread"])
def test_ms_roi_align_config_f_full_size_vs_oracle(ops, regime):
    """VERDICT r4 "next" 6: MultiScaleRoIAlign (models/new_model.py:127,143) at config F's REAL shape -- 256 channels x {200x336, 100x168, 50x84,
    25x42}, 512 RoIs on an 800 x 1344 frame -- forward (roi_align_fwd77_kernel) bit for bit and backward (lists -> plan -> tile -> combine) within
    1e-5 of the scale against the C oracle.  'proposal_like' = what the head's sampler hands over after NMS (many small boxes, all four levels);
    'spread' = uniformly sized boxes up to the whole frame (large footprints, split tiles, every level mapped)."""
    rng = np.random.RandomState(11 if regime == "spread" else 12)
    C, R, Wimg, Himg = 256, 512, 1344, 800
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42)]
    feats = [rng.randn(C, h, w).astype(np.float32) for h, w in shapes]
    if regime == "spread":
        rois = rand_boxes(rng, R, 0.01, 0.98)
    else:
        c = rng.uniform(0.05, 0.95, (R, 2)).astype(np.float32)
        wh = np.exp(rng.uniform(np.log(0.02), np.log(0.7), (R, 2))).astype(np.float32)
        rois = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)
    rois = (rois * np.array([Wimg, Himg, Wimg, Himg], np.float32)).astype(np.float32)
    rois[0] = [-30, -20, 180, 150]                        # partly outside the frame
    rois[1] = [1300, 760, 1360, 820]
    rois[2] = [0, 0, Wimg, Himg]                          # the whole frame: the coarsest level, the largest footprint
    out_o, lv = orc.ms_roi_align(feats, rois)
    assert set(lv.tolist()) == {0, 1, 2, 3}
    fts = [T(f[None]).requires_grad_(True) for f in feats]
    m = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    out = m({str(i): f for i, f in enumerate(fts)}, [T(rois)], [(Wimg, Himg)])
    assert np.array_equal(ops.roi_level_map(T(rois)).cpu().numpy(), lv)
    assert np.array_equal(out.detach().cpu().numpy(), out_o)                     # the forward follows the oracle's operation order: bit-exact
    go = rng.randn(*out_o.shape).astype(np.float32)
    out.backward(T(go))
    worst = 0.0
    for l, f in enumerate(fts):
        gf_o = orc.roi_align_bwd(go, feats[l].shape, rois, 0.25 / (1 << l), 2, False, lv, l)
        d = float(np.abs(f.grad[0].cpu().numpy() - gf_o).max()) / max(1.0, float(np.abs(gf_o).max()))
        worst = max(worst, d)
    assert worst < 1e-5, worst                                                   # a different (fixed) summation order than the oracle's scatter


@pytest.mark.parametrize("PH,SR", [(7, 2), (5, 3), (7, 0)])
def test_single_level_roi_align_big_footprints_and_generic_shapes(ops, PH, SR):
    """One level of 300 x 260 at scale 1: RoIs whose footprint exceeds the forward staging buffer (fh*fw > 8192) and the
    backward row table (fh > 256) must take the in-kernel gather/scatter fallbacks; other bin/sampling shapes the generic kernels."""
    rng = np.random.RandomState(PH * 10 + SR)
    C, H, W = 20, 300, 260
    f = rng.randn(C, H, W).astype(np.float32)
    rois = rand_boxes(rng, 40, 0.02, 0.5) * np.array([W, H, W, H], np.float32)
    rois[0] = [0, 0, W, H]                                   # whole map: fh = 300 > 256, fp = 78 000
    rois[1] = [-20, -30, W + 25, H + 40]                     # sticks out on all sides (samples beyond [-1, H] contribute 0)
    rois[2] = [10, 5, 250, 100]                              # fp = 96 x 241 > 8192, fh < 256
    rois[3] = [100.5, 100.5, 100.7, 100.6]                   # tiny (clamped to 1 x 1)
    rois[4] = [W - 1.5, H - 1.5, W + 3, H + 3]               # bottom-right corner clamp
    out_o = orc.roi_align_fwd(f, rois, PH, PH, 1.0, SR, False)
    ft = T(f[None]).requires_grad_(True)
    out = ops.ms_roi_align([ft], T(rois), PH, SR, scales=(1.0,))
    assert np.abs(out.detach().cpu().numpy() - out_o).max() < 1e-5
    go = rng.randn(*out_o.shape).astype(np.float32)
    out.backward(T(go))
    gf_o = orc.roi_align_bwd(go, f.shape, rois, 1.0, SR, False)
    assert np.allclose(ft.grad[0].cpu().numpy(), gf_o, rtol=1e-4, atol=2e-4)


def test_ms_roi_align_bwd_plan_coarsens_when_the_item_table_is_too_small(ops):
    """One level, 512 RoIs that each cover most of a 50 x 84 map: every one of the 44 tiles meets hundreds of RoIs, which asks for
    far more list segments than the work-item table holds (tiles + 15 R / 32 + 1).  The planning step (the last workgroup of
    roi_align_bwd_lists_kernel) must double the split threshold until the plan fits -- and the gradient must still be the oracle's, bit-reproducibly."""
    from faster_rcnn_pytorch_amd import _lib
    import ctypes as C
    rng = np.random.RandomState(9)
    Cc, Hh, Ww, R = 64, 50, 84, 512
    c = rng.rand(R, 2).astype(np.float32) * 0.2 + 0.4
    wh = rng.rand(R, 2).astype(np.float32) * 0.3 + 0.6
    rois = (np.concatenate([c - wh / 2, c + wh / 2], 1).clip(0, 1) * np.array([Ww, Hh, Ww, Hh], np.float32) * 16.0).astype(np.float32)
    go = rng.randn(R, Cc, 7, 7).astype(np.float32)
    H = np.array([Hh], np.int32); W = np.array([Ww], np.int32); sc = np.array([1.0 / 16.0], np.float32)

    def run():
        g = torch.full((Cc, Hh, Ww), 3.0, dtype=torch.float32, device=DEV)
        ptrs = (C.c_void_p * 1)(g.data_ptr())
        nb = _lib.lib.frcnn_ms_roi_align_bwd_workspace(H.ctypes.data, W.ctypes.data, 1, Cc, R)
        ws = torch.full((max(nb, 256),), 0xA5, dtype=torch.uint8, device=DEV)
        _lib.check(_lib.lib.frcnn_ms_roi_align_bwd(T(go).data_ptr(), ptrs, H.ctypes.data, W.ctypes.data, sc.ctypes.data, 1, Cc, T(rois).data_ptr(), R,
                                                   7, 7, 2, 0, 4, 224.0, 4, ws.data_ptr(), ws.numel(), None), "bwd")
        torch.cuda.synchronize()
        return g.cpu().numpy()
    a, b = run(), run()
    assert np.array_equal(a, b)
    ref = orc.roi_align_bwd(go, (Cc, Hh, Ww), rois, 1.0 / 16.0, 2, False)
    assert np.allclose(a, ref, rtol=2e-4, atol=2e-3), float(np.abs(a - ref).max())


def test_ms_roi_align_bwd_records_and_in_kernel_tables_give_the_same_bits(ops):
    """The weight tables of a (RoI, tile) pair are built once by the lists launch and fetched by the tile kernel as 1 KB records; a RoI
    whose footprint spans more than 16 tiles -- or every RoI, with FRCNN_RA_RECORDS=0 (read once per process: a child process) -- has
    them built inside the tile kernel by the same function.  Same bits either way, on the DMA (C = 256) and the register (C = 40) path."""
    import os, subprocess, sys, tempfile
    rng = np.random.RandomState(17)
    code = ("import numpy as np, torch, sys; from faster_rcnn_pytorch_amd import ops; d = sys.argv[1]; C = int(sys.argv[2]);"
            "rois = torch.from_numpy(np.load(d + '/rois.npy')).cuda(); go = torch.from_numpy(np.load(d + '/go%d.npy' % C)).cuda();"
            "fts = [torch.zeros((1, C, h, w), device='cuda', requires_grad=True) for h, w in ((100, 168), (50, 84), (25, 42), (13, 21))];"
            "ops.ms_roi_align(fts, rois, 7, 2).backward(go);"
            "np.save(d + '/g%d.npy' % C, np.concatenate([f.grad.cpu().numpy().ravel() for f in fts]))")
    rois = rand_boxes(rng, 200, 0.02, 0.7) * np.array([672, 400, 672, 400], np.float32)
    rois[:8] = [[0, 0, 672, 400]] * 8                                             # whole image on the coarsest level: 2 x 3 tiles
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "rois.npy"), rois)
        for Cc in (256, 40):
            go = rng.randn(200, Cc, 7, 7).astype(np.float32)
            np.save(os.path.join(d, "go%d.npy" % Cc), go)
            fts = [torch.zeros((1, Cc, h, w), device=DEV, requires_grad=True) for h, w in ((100, 168), (50, 84), (25, 42), (13, 21))]
            ops.ms_roi_align(fts, T(rois), 7, 2).backward(T(go))
            here = np.concatenate([f.grad.cpu().numpy().ravel() for f in fts])
            env = dict(os.environ, FRCNN_RA_RECORDS="0", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            subprocess.run([sys.executable, "-c", code, d, str(Cc)], check=True, env=env, timeout=300)
            assert np.array_equal(np.load(os.path.join(d, "g%d.npy" % Cc)), here), Cc


def test_ms_roi_align_bwd_mixed_record_and_in_kernel_tables_on_the_dma_path(ops):
    """One 50 x 84 level, C = 64 (whole channel groups: the LDS-DMA instantiation of the tile kernel): small RoIs have records, RoIs
    spanning more than 16 tiles have their tables built by wave 3 of the tile kernel -- in the same lists, so the counted vmcnt waits see
    both kinds of predecessor (two or one outstanding transfer).  Gradient = the oracle's."""
    rng = np.random.RandomState(29)
    Cc, Hh, Ww = 64, 50, 84
    small = rand_boxes(rng, 120, 0.03, 0.25) * np.array([Ww, Hh, Ww, Hh], np.float32) * 16.0
    big = rand_boxes(rng, 40, 0.6, 0.95) * np.array([Ww, Hh, Ww, Hh], np.float32) * 16.0
    rois = np.concatenate([small, big])[rng.permutation(160)].astype(np.float32)
    go = rng.randn(160, Cc, 7, 7).astype(np.float32)
    ft = torch.zeros((1, Cc, Hh, Ww), device=DEV, requires_grad=True)
    ops.ms_roi_align([ft], T(rois), 7, 2, scales=(1.0 / 16.0,)).backward(T(go))
    ref = orc.roi_align_bwd(go, (Cc, Hh, Ww), rois, 1.0 / 16.0, 2, False)
    assert np.allclose(ft.grad[0].cpu().numpy(), ref, rtol=2e-4, atol=1e-3), float(np.abs(ft.grad[0].cpu().numpy() - ref).max())


def test_ms_roi_align_bwd_tile_gather_is_reproducible_and_overwrites(ops):
    """The 7x7 / sampling-ratio-2 backward owns tiles instead of scattering atomics: two runs give identical bits, stale
    contents of the gradient buffers do not leak (the library overwrites), clustered RoIs (64 on one spot) and R = 0 work."""
    from faster_rcnn_pytorch_amd import _lib
    import ctypes as C
    rng = np.random.RandomState(3)
    shapes = [(256, 100, 168), (256, 50, 84), (256, 25, 42), (256, 13, 21)]
    rois = rand_boxes(rng, 300, 0.02, 0.6) * np.array([672, 400, 672, 400], np.float32)
    rois[:64] = rois[0] + rng.randn(64, 4).astype(np.float32) * 2.0               # a pile of near-identical RoIs on one tile
    go = rng.randn(300, 256, 7, 7).astype(np.float32)
    lv = orc.roi_level_map(rois)
    H = np.array([s[1] for s in shapes], np.int32); W = np.array([s[2] for s in shapes], np.int32)
    sc = np.array([0.25, 0.125, 0.0625, 0.03125], np.float32)

    def run(fill, R):
        grads = [torch.full(s, fill, dtype=torch.float32, device=DEV) for s in shapes]
        ptrs = (C.c_void_p * 4)(*[g.data_ptr() for g in grads])
        nb = _lib.lib.frcnn_ms_roi_align_bwd_workspace(H.ctypes.data, W.ctypes.data, 4, 256, R)
        ws = torch.full((max(nb, 256),), 0x5A, dtype=torch.uint8, device=DEV)     # stale bytes in the workspace must not matter
        _lib.check(_lib.lib.frcnn_ms_roi_align_bwd(T(go).data_ptr(), ptrs, H.ctypes.data, W.ctypes.data, sc.ctypes.data, 4, 256, T(rois).data_ptr(), R,
                                                   7, 7, 2, 0, 2, 224.0, 4, ws.data_ptr(), ws.numel(), None), "bwd")
        torch.cuda.synchronize()
        return [g.cpu().numpy() for g in grads]
    a, b = run(0.0, 300), run(123.0, 300)
    for l in range(4):
        assert np.array_equal(a[l], b[l])                                          # overwritten + bit-reproducible
        ref = orc.roi_align_bwd(go, shapes[l], rois, float(sc[l]), 2, False, lv, l)
        assert np.allclose(a[l], ref, rtol=1e-4, atol=2e-4)
    z = run(7.0, 0)
    assert all((g == 0).all() for g in z)                                          # no RoIs: zero gradient, not stale memory


# ------------------------------------------------------------------------------------------ RPN head tail (MFMA)
@pytest.mark.parametrize("C,fh,fw,A", [(512, 37, 62, 9), (256, 50, 84, 3), (64, 5, 7, 9)])
def test_rpn_head_tail_vs_torch_fp32(ops, C, fh, fw, A):
    """Floating-point kernel: compared with the plain fp32 op chain of models/model.py:79-83 (torch CPU, float64 check),
    tolerance 1e-5 absolute on outputs of magnitude ~0.1 (north star: 1e-4)."""
    g = torch.Generator().manual_seed(C + A)
    raw = torch.randn(1, C, fh, fw, generator=g)
    b3 = torch.randn(C, generator=g) * 0.1
    wc = torch.randn(2 * A, C, 1, 1, generator=g) * 0.02
    bc = torch.randn(2 * A, generator=g) * 0.1
    wr = torch.randn(4 * A, C, 1, 1, generator=g) * 0.02
    br = torch.randn(4 * A, generator=g) * 0.1
    h = torch.relu(raw.double() + b3.double()[None, :, None, None])
    ref_cls = torch.nn.functional.conv2d(h, wc.double(), bc.double()).permute(0, 2, 3, 1).contiguous().view(1, -1, 2)
    ref_reg = torch.nn.functional.conv2d(h, wr.double(), br.double()).permute(0, 2, 3, 1).contiguous().view(1, -1, 4)
    args = [t.to(DEV).requires_grad_(True) for t in (raw, b3, wc, bc, wr, br)]
    cls, reg = ops.rpn_head_tail(*args)
    assert cls.shape == ref_cls.shape and reg.shape == ref_reg.shape
    assert (cls.detach().cpu().double() - ref_cls).abs().max() < 1e-5
    assert (reg.detach().cpu().double() - ref_reg).abs().max() < 1e-5
    # backward against autograd of the reference op chain (the fused backward exists for the reference's widths, 256 and 512)
    gc, gr = torch.randn(cls.shape, generator=g), torch.randn(reg.shape, generator=g)
    if C not in (256, 512):
        from faster_rcnn_pytorch_amd._lib import FrcnnError
        with pytest.raises(FrcnnError, match="head widths"):
            (cls * gc.to(DEV)).sum().backward()
        return
    (cls * gc.to(DEV)).sum().backward(retain_graph=True)
    (reg * gr.to(DEV)).sum().backward()
    ref_in = [t.clone().double().requires_grad_(True) for t in (raw, b3, wc, bc, wr, br)]
    h2 = torch.relu(ref_in[0] + ref_in[1][None, :, None, None])
    c2 = torch.nn.functional.conv2d(h2, ref_in[2], ref_in[3]).permute(0, 2, 3, 1).contiguous().view(1, -1, 2)
    r2 = torch.nn.functional.conv2d(h2, ref_in[4], ref_in[5]).permute(0, 2, 3, 1).contiguous().view(1, -1, 4)
    ((c2 * gc.double()).sum() + (r2 * gr.double()).sum()).backward()
    for a, b in zip(args, ref_in):
        assert (a.grad.cpu().double() - b.grad).abs().max() < 2e-4 * max(1.0, float(b.grad.abs().max()))


@pytest.mark.parametrize("dtype,mfma,tol", [("f32", "f32", 1e-5), ("f32", "bf16", 2e-2), ("bf16", "bf16", 2e-2), ("bf16", "f32", 1e-5)])
def test_rpn_head_tail_all_fpn_levels_one_launch(ops, dtype, mfma, tol):
    """The shared FPN head (new_model.py:37-44,109-113: A = 3, C = 256, five levels) in one launch, fp32 and the mixed
    precision forms.  Reference: the plain op chain in float64 on the SAME (possibly bf16-rounded) conv outputs.  Tolerances:
    exact-fp32 MFMA 1e-5 absolute; bf16 operands (8 mantissa bits, K = 256, |out| ~ 0.3) 2e-2 absolute."""
    g = torch.Generator().manual_seed(11)
    C_, A = 256, 3
    shapes = [(40, 56), (20, 28), (10, 14), (5, 7), (3, 4)]
    raws = [torch.randn(1, C_, h, w, generator=g) for h, w in shapes]
    if dtype == "bf16":
        raws = [r.bfloat16() for r in raws]
    b3 = torch.randn(C_, generator=g) * 0.1
    wc, bc = torch.randn(2 * A, C_, 1, 1, generator=g) * 0.02, torch.randn(2 * A, generator=g) * 0.1
    wr, br = torch.randn(4 * A, C_, 1, 1, generator=g) * 0.02, torch.randn(4 * A, generator=g) * 0.1
    ref_c, ref_r = [], []
    for r in raws:
        h = torch.relu(r.double() + b3.double()[None, :, None, None])
        ref_c.append(torch.nn.functional.conv2d(h, wc.double(), bc.double()).permute(0, 2, 3, 1).contiguous().view(1, -1, 2))
        ref_r.append(torch.nn.functional.conv2d(h, wr.double(), br.double()).permute(0, 2, 3, 1).contiguous().view(1, -1, 4))
    ref_c, ref_r = torch.cat(ref_c, 1), torch.cat(ref_r, 1)
    dr = [r.to(DEV).requires_grad_(True) for r in raws]
    params = [t.to(DEV).requires_grad_(True) for t in (b3, wc, bc, wr, br)]
    cls, reg = ops.rpn_head_tail_levels(dr, *params, mfma=mfma)
    assert cls.dtype == torch.float32 and reg.dtype == torch.float32                  # box regression stays fp32
    assert cls.shape == ref_c.shape and reg.shape == ref_r.shape
    assert (cls.detach().cpu().double() - ref_c).abs().max() < tol and (reg.detach().cpu().double() - ref_r).abs().max() < tol
    if mfma == "f32" and dtype == "f32":                                             # one level through the old entry point: identical bits
        c1, r1 = ops.rpn_head_tail(dr[1].detach(), *[p.detach() for p in params])
        n0, n1 = shapes[0][0] * shapes[0][1] * A, shapes[1][0] * shapes[1][1] * A
        assert torch.equal(c1[0], cls[0, n0:n0 + n1].detach()) and torch.equal(r1[0], reg[0, n0:n0 + n1].detach())
    # backward (fp32 torch ops on recomputed activations) against float64 autograd of the op chain
    gc, gr = torch.randn(cls.shape, generator=g), torch.randn(reg.shape, generator=g)
    ((cls * gc.to(DEV)).sum() + (reg * gr.to(DEV)).sum()).backward()
    ref_in = [r.double().requires_grad_(True) for r in raws] + [t.clone().double().requires_grad_(True) for t in (b3, wc, bc, wr, br)]
    cc, rr = [], []
    for r in ref_in[:5]:
        h = torch.relu(r + ref_in[5][None, :, None, None])
        cc.append(torch.nn.functional.conv2d(h, ref_in[6], ref_in[7]).permute(0, 2, 3, 1).contiguous().view(1, -1, 2))
        rr.append(torch.nn.functional.conv2d(h, ref_in[8], ref_in[9]).permute(0, 2, 3, 1).contiguous().view(1, -1, 4))
    ((torch.cat(cc, 1) * gc.double()).sum() + (torch.cat(rr, 1) * gr.double()).sum()).backward()
    btol = 2e-4 if dtype == "f32" else 1e-2                                           # bf16 leaf: its gradient is rounded to bf16
    for a, b in zip(dr + params, ref_in):
        assert a.grad.dtype == a.dtype
        assert (a.grad.cpu().double() - b.grad).abs().max() < btol * max(1.0, float(b.grad.abs().max()))


# ------------------------------------------------------------------------------------------ edge cases (empty / ragged / extreme sizes)
def test_empty_and_degenerate_inputs(ops):
    e4 = torch.zeros((0, 4), device=DEV)
    e1 = torch.zeros((0,), device=DEV)
    assert ops.nms(e4, e1, 0.5).shape == (0,)
    assert ops.xy_to_cxcy(e4).shape == (0, 4)
    assert ops.find_jaccard_overlap(e4, T(np.array([[0, 0, 1, 1]], np.float32))).shape == (0, 1)
    one = T(np.array([[0.1, 0.1, 0.4, 0.5]], np.float32))
    assert ops.nms(one, T(np.array([0.3], np.float32)), 0.5).cpu().tolist() == [0]
    # RoIPool with zero RoIs: empty output, zero gradient
    f = torch.randn(1, 8, 5, 6, device=DEV, requires_grad=True)
    out = ops.roi_pool(f, e4, (7, 7), 1.0)
    assert out.shape == (0, 8, 7, 7)
    # every box filtered by min_size: zero proposals, count 0, no crash downstream
    anchor = orc.anchor_grid(160, 240)
    N = anchor.shape[0]
    reg = np.zeros((N, 4), np.float32)
    reg[:, 2:] = -30.0                                          # all boxes collapse
    cls = np.zeros((N, 2), np.float32)
    rois, cnt, _ = ops.region_proposal(T(reg), T(cls), T(anchor), 1 / 1000, 12000, 0.7, 2000)
    assert int(cnt.item()) == 0 and orc.region_proposal(reg, cls, anchor, 1 / 1000, 12000, 0.7, 2000)[0].shape[0] == 0
    # head targets with zero live proposals: candidates are the GT boxes alone (model_.py:135): 3 rows of 128.  The reference
    # throws here (model.py:340); the library flags it (SHORT) and marks the unfilled rows with the out-of-range class -1
    from faster_rcnn_pytorch_amd import _lib
    gt = _gt(np.random.RandomState(0), 3)
    lab = np.array([1, 2, 3], np.int64)
    cls_t, reg_t, srois, keep, counts = ops.head_targets(rois, T(gt), T(lab), n_rois=cnt, seed=1, want_keep=True)
    c = counts.cpu().tolist()
    assert c[0] == 3 and c[1] == 0 and c[2] == 3 and c[3] == _lib.HT_ERR_SHORT
    k = keep.cpu().numpy()
    assert sorted(k[:3].tolist()) == [0, 1, 2] and (k[3:] == -1).all() and (cls_t.cpu().numpy()[3:] == -1).all()
    assert (cls_t.cpu().numpy()[:3] >= 1).all()


def test_upstream_abort_and_short_samples_surface_without_a_sync(ops, golden):
    """VERDICT r1 #7 / ADVICE r1: a scan abort upstream (device count -1) or fewer than `total` samples must not silently
    become a GT-only / fake-background step.  Forged counts (no real abort is provoked): error bits in counts[3], sticky
    status word, class -1 rows, NaN loss, DeviceStatus.check() raises."""
    from faster_rcnn_pytorch_amd import _lib
    rng = np.random.RandomState(5)
    gt = _gt(rng, 3)
    lab = np.array([4, 5, 6], np.int64)
    rois = rand_boxes(rng, 2000, 0.05, 0.5)
    st = ops.DeviceStatus()
    word = st.word(torch.device(DEV))
    # 1. healthy call: no bits, word stays clean
    out = ops.head_targets(T(rois), T(gt), T(lab), n_rois=T(np.array([2000], np.int32)), seed=1, status=word)
    assert out[4].cpu().tolist()[3] == 0 and int(word.item()) == 0 and (out[0].cpu().numpy() >= 0).all()
    st.check()
    # 2. forged upstream abort
    out = ops.head_targets(T(rois), T(gt), T(lab), n_rois=T(np.array([-1], np.int32)), seed=1, status=word)
    c = out[4].cpu().tolist()
    assert c[3] & _lib.HT_ERR_UPSTREAM_ABORT
    assert (out[0].cpu().numpy() == -1).all()                                 # every row carries the failure mark
    assert int(word.item()) & _lib.HT_ERR_UPSTREAM_ABORT
    # ... a later healthy step does not clear the sticky word
    ops.head_targets(T(rois), T(gt), T(lab), n_rois=T(np.array([2000], np.int32)), seed=2, status=word)
    assert int(word.item()) & _lib.HT_ERR_UPSTREAM_ABORT
    with pytest.raises(_lib.FrcnnError, match="aborted NMS scan"):
        st.check()
    st.check()                                                                # cleared by the raise
    # 3. the loss of such a step is NaN (total and head CE), found at the caller's loss.item()
    g = golden("loss")
    pred = tuple(T(g[k]) for k in ("p_rpn_cls", "p_rpn_reg", "p_head_cls", "p_head_reg"))
    tgt = [T(g[k]) for k in ("t_rpn_cls", "t_rpn_reg", "t_head_cls", "t_head_reg")]
    ok = ops.detection_loss(pred, tgt)
    assert all(np.isfinite(float(v)) for v in ok)
    tgt[2] = torch.full_like(tgt[2], -1)
    bad = ops.detection_loss(pred, tgt)
    assert np.isnan(float(bad[0])) and np.isnan(float(bad[3])) and np.isfinite(float(bad[1]))
    tgt[2] = T(g["t_head_cls"]).clone()
    tgt[2][7] = 21                                                            # one row out of range (NC = 21) is enough
    assert np.isnan(float(ops.detection_loss(pred, tgt)[0]))
    # 4. fewer candidates than `total`: P + G < 128
    out = ops.head_targets(T(rois[:40]), T(gt), T(lab), seed=1, status=word, want_keep=True)
    c = out[4].cpu().tolist()
    assert c[3] == _lib.HT_ERR_SHORT and c[2] == c[0] + c[1] < 128
    cls = out[0].cpu().numpy()
    assert (cls[:c[2]] >= 0).all() and (cls[c[2]:] == -1).all()
    with pytest.raises(_lib.FrcnnError, match="fewer RoI samples"):
        st.check()


def test_anchor_generator_call_convention_of_the_reference(ops):
    """models/new_model.py:46-47: anchor = self.anchor_generator(ImageList(x, [(w, h)]), features)[0]; anchor /= (w, h, w, h)."""
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    feats = {str(i): torch.zeros(1, 2, fh, fw, device=DEV) for i, (fh, fw) in enumerate(shapes)}
    x = torch.zeros(1, 3, 800, 1344, device=DEV)
    ag = ops.AnchorGenerator()
    a = ag(ops.ImageList(x, [(1344, 800)]), feats)[0]
    want = orc.tv_anchor_grid(800, 1344, shapes, normalise=False)
    assert np.array_equal(a.cpu().numpy(), want)
    a /= torch.tensor([1344, 800, 1344, 800], dtype=torch.float32, device=DEV)      # the reference's in-place normalisation
    assert np.array_equal(a.cpu().numpy(), orc.tv_anchor_grid(800, 1344, shapes, normalise=True))
    # ... must not have touched the cached grid: a second call still returns pixels
    assert np.array_equal(ag(ops.ImageList(x, [(1344, 800)]), list(feats.values()))[0].cpu().numpy(), want)
    assert np.array_equal(ag((800, 1344), list(feats.values()))[0].cpu().numpy(), want)


def test_ms_roi_align_reference_scale_mode(ops):
    """scales='reference' = torchvision's scale inference fed with the reference's swapped [(w, h)] (new_model.py:143): on an
    800x1344 frame the four maps are pooled at 1/8 .. 1/64 with level mapper k_min 3."""
    rng = np.random.RandomState(3)
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42)]
    feats = [rng.randn(1, 8, fh, fw).astype(np.float32) for fh, fw in shapes]
    fd = {str(i): T(f) for i, f in enumerate(feats)}
    rois = rand_boxes(rng, 64, 0.03, 0.9) * np.array([1344, 800, 1344, 800], np.float32)
    got = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2, scales="reference")(fd, [T(rois)], [(1344, 800)]).cpu().numpy()
    sc = (1 / 8, 1 / 16, 1 / 32, 1 / 64)
    want, lv = orc.ms_roi_align([f[0] for f in feats], rois, scales=sc)
    assert len(np.unique(lv)) >= 3
    assert np.abs(got - want).max() < 1e-5
    dflt = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)(fd, [T(rois)], [(1344, 800)]).cpu().numpy()
    assert np.abs(dflt - got).max() > 1e-3                                   # the two conventions really differ on this frame


@pytest.mark.parametrize("K", [300, 12000, 20000])
def test_nms_zero_live_boxes_writes_a_zero_count(ops, K):
    """A device-side live count of 0 (an image whose proposals were all filtered): no resolver workgroup runs, so nobody takes the
    ticket that writes the outputs -- the count must still come out as 0 (dense form: block 0 writes it; cascade: nms_emit)."""
    rng = np.random.RandomState(3)
    b = rand_boxes(rng, K, 0.05, 0.3)
    cnt = ops.nms_sorted(T(b), 0.7, post_k=min(K, 2000), n_boxes=T(np.array([0], np.int32)))[2]
    assert int(cnt.item()) == 0
    cnt = ops.nms_sorted(T(b), 0.7, post_k=min(K, 2000), n_boxes=T(np.array([K], np.int32)))[2]        # and the workspace is fine afterwards
    assert int(cnt.item()) == min(len(orc.nms(b, 0.7)), 2000)


def test_nms_all_identical_boxes_and_single_survivor(ops):
    K = 5000
    b = np.tile(np.array([[0.2, 0.2, 0.6, 0.7]], np.float32), (K, 1))
    keep, _, cnt = ops.nms_sorted(T(b), 0.7)
    assert int(cnt.item()) == 1 and int(keep[0]) == 0             # IoU = 1 > thr: only the first survives
    disjoint = np.zeros((K, 4), np.float32)                       # nobody overlaps: everyone survives, in order
    g = np.arange(K)
    disjoint[:, 0] = (g % 100) * 0.01
    disjoint[:, 1] = (g // 100) * 0.01
    disjoint[:, 2] = disjoint[:, 0] + 0.005
    disjoint[:, 3] = disjoint[:, 1] + 0.005
    keep, _, cnt = ops.nms_sorted(T(disjoint), 0.3)
    assert int(cnt.item()) == K and np.array_equal(keep.cpu().numpy(), np.arange(K))


def test_nms_above_fast_path_limit_uses_generic_scan(ops):
    rng = np.random.RandomState(1)
    K = 13000                                                     # > 12288: the unpipelined scan
    c = rng.rand(K, 2).astype(np.float32) * 0.7 + 0.15
    wh = rng.rand(K, 2).astype(np.float32) * 0.2 + 0.03
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    keep_o = orc.nms(b, 0.6)
    keep, _, cnt = ops.nms_sorted(T(b), 0.6)
    assert int(cnt.item()) == len(keep_o) and np.array_equal(keep[:len(keep_o)].cpu().numpy(), keep_o)


def test_nms_two_launch_form_for_very_large_k():
    """Above FRCNN_NMS_FUSED_MAX_RES resolver workgroups (1024 = K > 65 536) nms_kernel runs as two launches (tiles, then resolver)
    instead of one.  The limit is read once per process, so a child process runs K = 3000 with the limit at 8."""
    import subprocess
    code = (
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from faster_rcnn_pytorch_amd import ops\n"
        "from oracle import oracle as orc\n"
        "rng = np.random.RandomState(4); K = 3000\n"
        "c = rng.rand(K, 2).astype(np.float32) * 0.7 + 0.15; wh = rng.rand(K, 2).astype(np.float32) * 0.25 + 0.03\n"
        "b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)\n"
        "ko = orc.nms(b, 0.5)\n"
        "keep, _, cnt = ops.nms_sorted(torch.from_numpy(b).cuda(), 0.5)\n"
        "assert int(cnt.item()) == len(ko) and np.array_equal(keep[:len(ko)].cpu().numpy(), ko)\n"
        "print('two-launch ok', len(ko))\n") % ROOT
    env = dict(os.environ, FRCNN_NMS_FUSED_MAX_RES="8")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "two-launch ok" in r.stdout, r.stdout + r.stderr


def test_rpn_targets_single_gt_and_gt_outside_all_anchors(ops):
    anchor = orc.anchor_grid(600, 1000)
    gt = np.array([[0.0, 0.0, 0.004, 0.004]], np.float32)         # tiny box: max IoU far below 0.3 -> only the forced match is positive
    cls_o, reg_o, (n_pos, n_neg) = orc.rpn_targets(anchor, gt)
    assert n_pos == 1
    pn = np.random.RandomState(0).permutation(n_neg)
    cls_o, _, _ = orc.rpn_targets(anchor, gt, None, pn)
    cls, _, counts = ops.rpn_targets(T(anchor), T(gt), perm_neg=pn)
    assert counts.cpu().tolist()[:3] == [1, n_neg, 0] and np.array_equal(cls.cpu().numpy(), cls_o)


def test_batched_nms_equals_per_class_loop(ops):
    """FRCNN._suppress (models/model.py:382-402): one class-aware NMS must reproduce the per-class nms(0.3) loop."""
    rng = np.random.RandomState(4)
    n, C = 4000, 20
    centers = rng.rand(30, 2).astype(np.float32) * 0.6 + 0.2
    c = centers[rng.randint(0, 30, n)] + rng.randn(n, 2).astype(np.float32) * 0.02
    wh = np.float32(0.2) + rng.randn(n, 2).astype(np.float32) * 0.03
    b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)
    sc = rng.rand(n).astype(np.float32)
    cl = rng.randint(0, C, n).astype(np.int64)
    keep = ops.batched_nms(T(b), T(sc), T(cl), 0.3).cpu().numpy()
    exp = []
    for l in range(C):
        m = np.nonzero(cl == l)[0]
        order = m[np.argsort(-sc[m], kind="stable")]
        exp.append(order[orc.nms(b[order], 0.3)])
    exp = np.concatenate(exp)
    assert sorted(keep.tolist()) == sorted(exp.tolist())                      # same survivors
    assert (np.diff(sc[keep]) <= 0).all()                                     # returned in global score order
    for l in range(C):                                                        # and per class in the per-class order
        assert np.array_equal(keep[cl[keep] == l], exp[cl[exp] == l])


# ------------------------------------------------------------------------------------------ fused detection loss (losses/loss.py:5-85)
def test_detection_loss_matches_reference_golden_and_autograd(ops, golden):
    """Floating-point kernel: values vs the reference's own FRCNNLoss (golden), gradients vs autograd of the torch fp32
    op chain of losses/loss.py; tolerance 2e-6 relative on the losses, 1e-6 absolute on the gradients."""
    from faster_rcnn_pytorch_amd.loss import FRCNNLoss
    from oracle.model_ref import ref_loss
    g = golden("loss")
    names_p = ("p_rpn_cls", "p_rpn_reg", "p_head_cls", "p_head_reg")
    names_t = ("t_rpn_cls", "t_rpn_reg", "t_head_cls", "t_head_reg")
    pred = [T(g[k]).requires_grad_(True) for k in names_p]
    target = [T(g[k]) for k in names_t]
    out = FRCNNLoss(None)(pred, target)                                       # dispatches to the HIP kernel on GPU tensors
    got = np.array([float(o) for o in out], np.float32)
    assert np.allclose(got, g["losses"], rtol=2e-6, atol=1e-6)
    (out[0] + 0.5 * out[2]).backward()
    ref_in = [torch.from_numpy(g[k]).clone().requires_grad_(True) for k in names_p]
    r = ref_loss(ref_in, [torch.from_numpy(g[k]) for k in names_t])
    (r[0] + 0.5 * r[2]).backward()
    for a, b in zip(pred, ref_in):
        assert (a.grad.cpu() - b.grad).abs().max() < 1e-6
    assert np.allclose(orc.frcnn_loss([g[k] for k in names_p], [g[k] for k in names_t]), g["losses"], rtol=2e-6, atol=1e-6)
    # the training step differentiates the total alone: three launches instead of seventeen, the same gradients bit for bit as the general form
    from faster_rcnn_pytorch_amd import _lib
    grads = []
    for general in (False, True):
        p2 = [T(g[k]).requires_grad_(True) for k in names_p]
        o2 = FRCNNLoss(None)(p2, target)
        (o2[0] + 0.0 * o2[1] if general else o2[0]).backward()
        grads.append([t.grad.clone() for t in p2])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    r2_in = [torch.from_numpy(g[k]).clone().requires_grad_(True) for k in names_p]
    ref_loss(r2_in, [torch.from_numpy(g[k]) for k in names_t])[0].backward()
    for a, b in zip(grads[0], r2_in):
        assert (a.cpu() - b.grad).abs().max() < 1e-6


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rpn_head_tail_backward_full_fpn_size_fused_vs_torch(ops, dtype):
    """The fused MFMA backward (csrc/rpn_head.hip) at the full FPN level shapes of 800x1344 (89 523 positions, C = 256, A = 3)
    against the same gradients from plain torch ops in float64 on the GPU.  Tolerances: d_raw 1e-5 absolute (fp32) / bf16 rounding
    (8 mantissa bits) of values ~0.05; dW / db / db3 are sums over 89 523 positions of terms ~1e-2: 1e-3 relative to their max."""
    g = torch.Generator().manual_seed(5)
    C_, A = 256, 3
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    raws = [torch.randn(1, C_, h, w, generator=g).to(DEV) for h, w in shapes]
    if dtype == "bf16":
        raws = [r.bfloat16() for r in raws]
    b3 = (torch.randn(C_, generator=g) * 0.1).to(DEV)
    wc, bc = (torch.randn(2 * A, C_, 1, 1, generator=g) * 0.02).to(DEV), (torch.randn(2 * A, generator=g) * 0.1).to(DEV)
    wr, br = (torch.randn(4 * A, C_, 1, 1, generator=g) * 0.02).to(DEV), (torch.randn(4 * A, generator=g) * 0.1).to(DEV)
    dr = [r.clone().requires_grad_(True) for r in raws]
    params = [t.clone().requires_grad_(True) for t in (b3, wc, bc, wr, br)]
    cls, reg = ops.rpn_head_tail_levels(dr, *params, mfma="f32")
    gc, gr = torch.randn(cls.shape, generator=g).to(DEV), torch.randn(reg.shape, generator=g).to(DEV)
    ((cls * gc).sum() + (reg * gr).sum()).backward()
    # float64 reference on the same (possibly bf16-rounded) conv outputs
    w_all = torch.cat([wc.reshape(2 * A, C_), wr.reshape(4 * A, C_)], 0).double()
    dW = torch.zeros(6 * A, C_, dtype=torch.float64, device=DEV)
    db = torch.zeros(6 * A, dtype=torch.float64, device=DEV)
    db3 = torch.zeros(C_, dtype=torch.float64, device=DEV)
    p0 = 0
    for r, d in zip(raws, dr):
        P = r.shape[2] * r.shape[3]
        gg = torch.cat([gc.reshape(-1, 2 * A)[p0:p0 + P], gr.reshape(-1, 4 * A)[p0:p0 + P]], 1).double()
        z = r.reshape(C_, P).double() + b3.double()[:, None]
        dz = (w_all.t() @ gg.t()) * (z > 0)
        dW += gg.t() @ torch.relu(z).t(); db += gg.sum(0); db3 += dz.sum(1)
        tol = 1e-5 if dtype == "f32" else 4e-3 * float(dz.abs().max())
        assert (d.grad.reshape(C_, P).double() - dz).abs().max() < tol
        p0 += P
    got_dW = torch.cat([params[1].grad.reshape(2 * A, C_), params[3].grad.reshape(4 * A, C_)], 0).double()
    got_db = torch.cat([params[2].grad, params[4].grad]).double()
    assert (got_dW - dW).abs().max() < 1e-3 * float(dW.abs().max())
    assert (got_db - db).abs().max() < 1e-3 * float(db.abs().max())
    assert (params[0].grad.double() - db3).abs().max() < 1e-3 * float(db3.abs().max())


@pytest.mark.parametrize("shapes", [[(40, 56), (20, 28), (10, 14), (5, 7), (3, 4)], [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)], [(9, 33)],
                                    [(104, 319), (12, 33)]])     # 134 tiles: more than half a round of CUs, so full 8-row tiles of ODD width
def test_rpn_conv_head_bf16_vs_torch(ops, shapes):
    """The fused bf16 implicit-GEMM RPN head (csrc/rpn_conv.hip; BASELINE configs[4]) against the plain op chain of
    models/new_model.py:109-113 in float64 on the SAME bf16-rounded inputs and weights.  Tolerances: raw is a K = 2304 bf16 dot
    product accumulated in fp32 then rounded to bf16 (|raw| ~ 0.5: 2^-8 relative = 4e-3 absolute); cls / reg read that bf16 raw and
    contract 256 bf16-rounded activations (2e-2 absolute, as the tail kernel's bf16 form).  Backward: against float64 autograd."""
    g = torch.Generator().manual_seed(21)
    C_, A = 256, 3
    feats = [(torch.randn(1, C_, h, w, generator=g)).bfloat16().to(DEV) for h, w in shapes]
    w3 = (torch.randn(C_, C_, 3, 3, generator=g) * 0.01).to(DEV)
    b3 = (torch.randn(C_, generator=g) * 0.1).to(DEV)
    wc, bc = (torch.randn(2 * A, C_, 1, 1, generator=g) * 0.02).to(DEV), (torch.randn(2 * A, generator=g) * 0.1).to(DEV)
    wr, br = (torch.randn(4 * A, C_, 1, 1, generator=g) * 0.02).to(DEV), (torch.randn(4 * A, generator=g) * 0.1).to(DEV)
    fin = [f.clone().requires_grad_(True) for f in feats]
    params = [t.clone().requires_grad_(True) for t in (w3, b3, wc, bc, wr, br)]
    cls, reg = ops.rpn_conv_head_levels(fin, *params)
    # float64 reference on bf16-rounded operands
    w3d = w3.bfloat16().double()
    rin = [f.double().requires_grad_(True) for f in feats]
    rp = [t.clone().double().requires_grad_(True) for t in (w3d, b3, wc.bfloat16().float(), bc, wr.bfloat16().float(), br)]
    cc, rr = [], []
    for f in rin:
        raw = torch.nn.functional.conv2d(f, rp[0], None, padding=1)
        h = torch.relu(raw + rp[1][None, :, None, None])
        cc.append(torch.nn.functional.conv2d(h, rp[2], rp[3]).permute(0, 2, 3, 1).contiguous().view(1, -1, 2))
        rr.append(torch.nn.functional.conv2d(h, rp[4], rp[5]).permute(0, 2, 3, 1).contiguous().view(1, -1, 4))
    ref_c, ref_r = torch.cat(cc, 1), torch.cat(rr, 1)
    assert cls.shape == ref_c.shape and reg.shape == ref_r.shape and cls.dtype == torch.float32
    assert (cls.detach().double() - ref_c.detach()).abs().max() < 2e-2 and (reg.detach().double() - ref_r.detach()).abs().max() < 2e-2
    gc, gr = torch.randn(cls.shape, generator=g).to(DEV), torch.randn(reg.shape, generator=g).to(DEV)
    ((cls * gc).sum() + (reg * gr).sum()).backward()
    ((ref_c * gc.double()).sum() + (ref_r * gr.double()).sum()).backward()
    for a, b in zip(fin, rin):                                       # bf16 data gradients
        assert (a.grad.double() - b.grad).abs().max() < 3e-2 * max(1.0, float(b.grad.abs().max()))
    for i, (a, b) in enumerate(zip(params, rp)):
        if i == 0:
            continue                                                 # w3: checked against the unfused mixed-precision path below
        # b3: the ReLU mask is decided on the bf16-rounded conv output, so a few positions with |raw + b3| < 2^-8 |raw| flip (8 %)
        tol = (8e-2 if i == 1 else 3e-2) * max(1e-3, float(b.grad.abs().max()))
        assert (a.grad.double() - b.grad).abs().max() < tol, (i, float((a.grad.double() - b.grad).abs().max()), float(b.grad.abs().max()))
    # ... and the fused launch agrees with the unfused mixed-precision path (MIOpen bf16 conv + the tail kernel) it replaces.  The
    # 3x3 weight gradient goes d_raw (bf16) -> MIOpen's bf16 weight-gradient kernel in BOTH paths; against float64 that carries up to
    # ~10 % of the largest entry (0.87 on 19.6 at the first shape set, identically for both paths), so it is pinned path against path.
    p2 = [t.clone().requires_grad_(True) for t in (w3, b3, wc, bc, wr, br)]
    raws2 = [torch.nn.functional.conv2d(f, p2[0].bfloat16(), None, padding=1) for f in feats]
    c2, r2 = ops.rpn_head_tail_levels(raws2, p2[1], p2[2], p2[3], p2[4], p2[5], mfma="bf16")
    ((c2 * gc).sum() + (r2 * gr).sum()).backward()
    assert (params[0].grad - p2[0].grad).abs().max() < 4e-2 * float(p2[0].grad.abs().max())       # a few bf16 ulps of the largest entry (MIOpen returns bf16)
    assert (cls.detach() - c2.detach()).abs().max() < 1e-2 and (reg.detach() - r2.detach()).abs().max() < 1e-2


@pytest.mark.parametrize("shapes", [[(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)], [(9, 33)], [(104, 319), (12, 33)]])
def test_rpn_conv_bwd_data_bf16_vs_torch(ops, shapes):
    """Backward-data of the 3x3 RPN convolution on the forward's implicit-GEMM kernel (transposed, flipped weights) against
    conv_transpose2d in float64 on the SAME bf16-rounded operands.  A K = 2304 bf16 dot product accumulated in fp32 and rounded to
    bf16: 2^-8 relative to the value (values ~0.5: 4e-3 absolute), odd widths and half tiles included."""
    g = torch.Generator().manual_seed(33)
    d_raws = [torch.randn(1, 256, h, w, generator=g).bfloat16().to(DEV) for h, w in shapes]
    w3 = (torch.randn(256, 256, 3, 3, generator=g) * 0.01).to(DEV)
    got = ops.rpn_conv_bwd_data(d_raws, w3)
    for d, o in zip(d_raws, got):
        ref = torch.nn.functional.conv_transpose2d(d.double(), w3.bfloat16().double(), padding=1)
        assert o.dtype == torch.bfloat16 and o.shape == d.shape
        err = (o.double() - ref).abs().max().item()
        assert err < 6e-3 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("shapes", [[(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)], [(9, 33)], [(104, 319), (12, 33)], [(3, 4)], [(70, 130), (5, 64)]])
def test_rpn_conv_wgrad_bf16_vs_torch(ops, shapes):
    """Weight gradient of the 3x3 RPN convolution (hand-written MFMA kernel, K split + fixed-order finalize) against float64 autograd on
    the SAME bf16-rounded operands.  Sums of up to 89 523 products of bf16 values accumulated in fp32: 1e-3 of the largest entry;
    reproducible bit for bit from run to run."""
    g = torch.Generator().manual_seed(44)
    feats = [torch.randn(1, 256, h, w, generator=g).bfloat16().to(DEV) for h, w in shapes]
    d_raws = [(torch.randn(1, 256, h, w, generator=g) * 0.1).bfloat16().to(DEV) for h, w in shapes]
    got = ops.rpn_conv_wgrad(feats, d_raws)
    w = torch.zeros(256, 256, 3, 3, dtype=torch.float64, device=DEV, requires_grad=True)
    tot = sum((torch.nn.functional.conv2d(f.double(), w, None, padding=1) * d.double()).sum() for f, d in zip(feats, d_raws))
    tot.backward()
    ref = w.grad
    err = (got.double() - ref).abs().max().item()
    assert err < 1e-3 * ref.abs().max().item(), (err, ref.abs().max().item())
    assert torch.equal(got, ops.rpn_conv_wgrad(feats, d_raws))


# ------------------------------------------------------------------------------------------ fp32 3x3 RPN conv (csrc/rpn_conv_f32.hip)
CONV_F32_CASES = [
    ("vgg600x1000", 512, [(37, 62)]),                                      # models/model.py:68-70 on the 600x1000 frame
    ("fpn800x1344", 256, [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]),   # models/new_model.py:96-98, five levels
    ("odd", 128, [(5, 7), (1, 1), (3, 130), (17, 2)]),                       # rows / columns shorter than a strip, a single pixel, a wrap inside a fragment
    ("one_tile", 256, [(8, 16)]),
]


def _conv_ref64(feats, w):
    import torch.nn.functional as F
    return [F.conv2d(f.double().cpu(), w.double().cpu(), None, padding=1) for f in feats]


@pytest.mark.parametrize("name,C,shapes", CONV_F32_CASES, ids=[c[0] for c in CONV_F32_CASES])
def test_rpn_conv3x3_f32_forward_backward_vs_float64(ops, name, C, shapes):
    """SURVEY A3 in the reference's precision: the hand-written fp32 MFMA 3x3 convolution (forward, data gradient, weight gradient)
    against a float64 evaluation of the same convolution on the CPU.  Tolerance 1e-4 of the output scale (north_star); measured
    ~1e-6: an fp32 fmaf chain over K = 9 C products.  Also: bit-reproducible run to run (fixed-order sums, no atomics on data)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(len(name) + C)
    feats = [torch.randn(1, C, h, w, generator=g) for h, w in shapes]
    wt = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    gouts = [torch.randn(1, C, h, w, generator=g) for h, w in shapes]
    fd = [f.to(DEV) for f in feats]
    gd = [t.to(DEV) for t in gouts]
    wd = wt.to(DEV)
    ref = _conv_ref64(feats, wt)
    from faster_rcnn_pytorch_amd import _lib
    _lib.prof_reset(); _lib.prof_enable(True)
    out = ops.rpn_conv3x3_fwd(fd, wd)
    _lib.prof_enable(False)
    assert "rpn_wino_gemm_kernel" in _lib.prof_report()                          # default form: Winograd F(2x2, 3x3), four launches
    for o, r in zip(out, ref):
        scale = float(r.abs().max())
        assert o.shape == r.shape and float((o.double().cpu() - r).abs().max()) < 1e-4 * max(1.0, scale)
        assert float((o.double().cpu() - r).abs().max()) < 2e-5 * max(1.0, scale)       # what an fp32 chain of this length really gives
    out2 = ops.rpn_conv3x3_fwd(fd, wd)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    # data gradient: d_feat = conv_transpose(d_out, w) = conv(d_out, w transposed and flipped)
    dref = [F.conv_transpose2d(t.double(), wt.double(), None, padding=1) for t in gouts]
    dgot = ops.rpn_conv3x3_bwd_data(gd, wd)
    for o, r in zip(dgot, dref):
        assert float((o.double().cpu() - r).abs().max()) < 2e-5 * max(1.0, float(r.abs().max()))
    assert all(torch.equal(a, b) for a, b in zip(dgot, ops.rpn_conv3x3_bwd_data(gd, wd)))
    # weight gradient, summed over the levels
    wref = torch.zeros(C, C, 3, 3, dtype=torch.float64)
    for f, t in zip(feats, gouts):
        wref += torch.nn.grad.conv2d_weight(f.double(), (C, C, 3, 3), t.double(), padding=1)
    wgot = ops.rpn_conv3x3_wgrad(fd, gd)
    err = float((wgot.double().cpu() - wref).abs().max())
    assert err < 1e-4 * max(1.0, float(wref.abs().max())), err
    assert torch.equal(wgot, ops.rpn_conv3x3_wgrad(fd, gd))


def test_rpn_conv3x3_f32_autograd_matches_torch_conv(ops):
    """The differentiable wrapper the two mirrors call (ops.rpn_conv3x3) against torch's own conv2d + autograd on the GPU (the vendor
    path it replaces): values and all three gradients within 1e-4 of the scale."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    C_ = 256
    shapes = [(24, 40), (12, 20), (6, 10)]
    feats = [torch.randn(1, C_, h, w, generator=g).to(DEV).requires_grad_(True) for h, w in shapes]
    wt = (torch.randn(C_, C_, 3, 3, generator=g) * 0.02).to(DEV).requires_grad_(True)
    gout = [torch.randn(1, C_, h, w, generator=g).to(DEV) for h, w in shapes]
    outs = ops.rpn_conv3x3(feats, wt)
    sum((o * t).sum() for o, t in zip(outs, gout)).backward()
    got = [f.grad.clone() for f in feats] + [wt.grad.clone()]
    for f in feats:
        f.grad = None
    wt.grad = None
    refs = [F.conv2d(f, wt, None, padding=1) for f in feats]
    sum((o * t).sum() for o, t in zip(refs, gout)).backward()
    for o, r in zip(outs, refs):
        assert float((o - r).abs().max()) < 1e-4 * max(1.0, float(r.abs().max()))
    for a, b in zip(got, [f.grad for f in feats] + [wt.grad]):
        assert float((a - b).abs().max()) < 1e-4 * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------ the same stage on the backbone's 3x3 convolutions
CONV3X3_CASES = [   # name, Cin, Cout, level shapes, bias, relu, gradients
    ("vgg_conv3_1", 128, 256, [(150, 250)], True, True, True),               # vgg16.features[10] + [11] behind models/model.py:279-281 at 600x1000
    ("vgg_conv4_1", 256, 512, [(75, 125)], True, True, True),                 # features[17] + [18]: odd rows and columns
    ("narrow_in", 64, 128, [(33, 47)], True, True, False),                    # Cin = 64 (features[5]): forward only
    ("wide_in", 384, 128, [(20, 31)], True, False, True),                     # Cin > Cout, bias without ReLU (the FPN's layer blocks)
    ("levels", 128, 128, [(9, 14), (30, 5), (1, 1)], False, True, True),      # several levels sharing the weight, no bias
    ("vgg_conv1_2", 64, 64, [(120, 200)], True, True, True),                  # features[2] + [3]: 64-wide tiles on both sides (F(4x4): 1500 tiles)
    ("vgg_conv2_1", 64, 128, [(100, 160)], True, True, True),                 # features[5] + [6]: a 64-channel input side
    ("narrow_both", 64, 64, [(20, 30), (7, 9)], True, True, True),            # the same with F(2x2)
    ("wide_out_64", 256, 64, [(25, 33)], True, False, True),                  # 64 outputs of a wide input
    ("rpn_37x62", 256, 128, [(37, 62)], True, True, True),                    # the RPN's / conv5's map at 600x1000: 160 4 x 4 tiles padded to 192 (64-wide product tiles)
    ("c5_25x42", 128, 128, [(25, 42)], False, True, True),                    # 273 2 x 2 tiles padded to 320: the 64-wide product tile with F(2x2)
    # the sizes bench.py runs: features[2] + [3] at 600 x 1000 = rpn_wino_gemm_out64_kernel forward and data gradient and the
    # k-contiguous 64 x 64-tile weight-gradient product with non-temporal operand transfers (commit 4d2cc32); features[5] + [6] at 300 x 500
    ("vgg_conv1_2_full", 64, 64, [(600, 1000)], True, True, True),
    ("vgg_conv2_1_full", 64, 128, [(300, 500)], True, True, True),
    ("resnet_layer1_full", 64, 64, [(200, 336)], True, True, True),           # layer1's conv2 at 800 x 1344 (the fused 64 -> 64 product on a second size)
]


@pytest.mark.parametrize("name,Cin,Cout,shapes,use_bias,relu,grads", CONV3X3_CASES, ids=[c[0] for c in CONV3X3_CASES])
def test_conv3x3_f32_stage_vs_float64(ops, name, Cin, Cout, shapes, use_bias, relu, grads):
    """frcnn_conv3x3_f32_fwd / _bwd_data / _wgrad (Cin != Cout, bias + ReLU in the output transform, the ReLU's backward in the gradient
    kernels' transforms, bias gradient) against float64 on the CPU.  The ReLU mask of the float64 gradients is taken from the DEVICE output:
    where the exact pre-activation is within rounding of zero the two forwards may legitimately disagree about the sign, and one such
    element moves a gradient by a whole dy * x; that the masks differ only there is asserted separately."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(len(name) * 7 + Cin)
    xs = [torch.randn(1, Cin, h, w, generator=g) for h, w in shapes]
    wt = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.2 if use_bias else None
    dys = [torch.randn(1, Cout, h, w, generator=g) for h, w in shapes]
    xd, dyd, wd = [x.to(DEV) for x in xs], [t.to(DEV) for t in dys], wt.to(DEV)
    bd = b.to(DEV) if use_bias else None
    pre = [F.conv2d(x.double(), wt.double(), b.double() if use_bias else None, padding=1) for x in xs]
    ys, _, bits = ops.conv3x3_fwd(xd, wd, bd, relu, want_bits=relu, keep_transformed=not relu)
    for y, p in zip(ys, pre):
        r = p.clamp_min(0) if relu else p
        assert y.shape == r.shape and float((y.double().cpu() - r).abs().max()) < 2e-5 * max(1.0, float(p.abs().max()))
    assert all(torch.equal(a, c) for a, c in zip(ys, ops.conv3x3_fwd(xd, wd, bd, relu)))          # bit-reproducible, with or without the extras
    if not grads:
        return
    masks = [(y.cpu() > 0) for y in ys] if relu else [torch.ones_like(p, dtype=torch.bool) for p in pre]
    for m, p in zip(masks if relu else [], pre):
        flips = m != (p > 0)
        assert int(flips.sum()) == 0 or float(p[flips].abs().max()) < 1e-5 * max(1.0, float(p.abs().max()))    # sign disagreements only at rounding-level zeros (of the output's scale, like the value bound above)
    gs = [t.double() * m for t, m in zip(dys, masks)]
    dx_ref = [F.conv_transpose2d(t, wt.double(), None, padding=1) for t in gs]
    dx = ops.conv3x3_bwd_data(dyd, wd, bits)
    for o, r in zip(dx, dx_ref):
        assert o.shape == r.shape and float((o.double().cpu() - r).abs().max()) < 2e-5 * max(1.0, float(r.abs().max()))
    assert all(torch.equal(a, c) for a, c in zip(dx, ops.conv3x3_bwd_data(dyd, wd, bits)))
    urot = ops.conv3x3_u_buffer(xd, wd)                                                          # the rotated weight transform made by the forward's launch
    ys_u = ops.conv3x3_fwd(xd, wd, bd, relu, u_rotated=urot)
    assert all(torch.equal(a, c) for a, c in zip(ys, ys_u))
    assert all(torch.equal(a, c) for a, c in zip(dx, ops.conv3x3_bwd_data(dyd, wd, bits, u_rotated=urot)))
    w_ref = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
    b_ref = torch.zeros(Cout, dtype=torch.float64)
    for x, t in zip(xs, gs):
        w_ref += torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), t, padding=1)
        b_ref += t.sum(dim=(0, 2, 3))
    dw, db = ops.conv3x3_wgrad(xd, dyd, bits, want_bias=True)
    assert float((dw.double().cpu() - w_ref).abs().max()) < 1e-4 * max(1.0, float(w_ref.abs().max()))
    assert float((db.double().cpu() - b_ref).abs().max()) < 1e-4 * max(1.0, float(b_ref.abs().max()))
    dw2, db2 = ops.conv3x3_wgrad(xd, dyd, bits, want_bias=True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    # the forward can keep its transformed activations for the weight gradient: same outputs, same gradient, one launch less
    ys_k, xt, _ = ops.conv3x3_fwd(xd, wd, bd, relu, keep_transformed=True)
    assert all(torch.equal(a, c) for a, c in zip(ys, ys_k))
    from faster_rcnn_pytorch_amd import _lib
    _lib.prof_reset(); _lib.prof_enable(True)
    dw3, db3 = ops.conv3x3_wgrad(xd, dyd, bits, want_bias=True, x_transformed=xt)
    _lib.prof_enable(False)
    assert torch.equal(dw, dw3) and torch.equal(db, db3)
    assert _lib.prof_report()["rpn_wino_input_kernel"][1] == 1                                     # only the output gradient was transformed
    # the data gradient's call can stage the output gradient once for both consumers: its own transform and the weight gradient's (+ bias partials)
    dyt = ops.conv3x3_dy_buffer(shapes, Cout, DEV)
    dx_s = ops.conv3x3_bwd_data(dyd, wd, bits, dy_transformed=dyt, want_bias_partials=True)
    _lib.prof_reset(); _lib.prof_enable(True)
    dw4, db4 = ops.conv3x3_wgrad(xd, dyd, bits, want_bias=True, x_transformed=xt, dy_transformed=dyt)
    _lib.prof_enable(False)
    assert all(torch.equal(a, c) for a, c in zip(dx, dx_s)) and torch.equal(dw, dw4) and torch.equal(db, db4)
    assert "rpn_wino_input_kernel" not in _lib.prof_report()                                       # nothing left to transform


SPLIT_CASES = [c for c in CONV3X3_CASES if c[0] in ("vgg_conv3_1", "vgg_conv4_1", "wide_in", "levels", "vgg_conv2_1", "narrow_both", "wide_out_64", "rpn_37x62")]
SPLIT_CASES += [("vgg_conv5_1", 512, 512, [(37, 62)], True, True, True)]           # Cin = 512: five of VGG16's thirteen convolutions are 512 -> 512


@pytest.mark.parametrize("name,Cin,Cout,shapes,use_bias,relu,grads", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_conv3x3_f32_split_products_are_as_close_to_float64_as_the_native_ones(ops, name, Cin, Cout, shapes, use_bias, relu, grads):
    """ops.conv3x3_f32_products("split"): the stage's products as six bf16 matrix instructions on exactly cut fp32 operands (csrc/rpn_conv_f32.hip, SPLIT).
    Forward, data gradient and weight gradient against float64 next to the native products' distance: within the native test's bounds, and never more than
    1.5 x the native distance (+ a rounding-level floor); bit-reproducible; the switch comes back as it was."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(len(name) * 7 + Cin)
    xs = [torch.randn(1, Cin, h, w, generator=g) for h, w in shapes]
    wt = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.2 if use_bias else None
    dys = [torch.randn(1, Cout, h, w, generator=g) for h, w in shapes]
    xd, dyd, wd = [x.to(DEV) for x in xs], [t.to(DEV) for t in dys], wt.to(DEV)
    bd = b.to(DEV) if use_bias else None
    pre = [F.conv2d(x.double(), wt.double(), b.double() if use_bias else None, padding=1) for x in xs]
    assert ops.conv3x3_f32_products() == "native"

    def run():
        ys, _, bits = ops.conv3x3_fwd(xd, wd, bd, relu, want_bits=relu, keep_transformed=not relu)
        dx = ops.conv3x3_bwd_data(dyd, wd, bits)
        dw, db = ops.conv3x3_wgrad(xd, dyd, bits, want_bias=True)
        return ys, bits, dx, dw, db
    nat = run()
    assert ops.conv3x3_f32_products("split") == "native"
    try:
        spl = run()
        again = run()
        assert ops.conv3x3_f32_products() == "split"
    finally:
        ops.conv3x3_f32_products("native")
    for a, c in zip(spl[0] + spl[2] + [spl[3], spl[4]], again[0] + again[2] + [again[3], again[4]]):
        assert torch.equal(a, c)                                                                  # bit-reproducible
    out = {}
    for tag, (ys, bits, dx, dw, db) in (("native", nat), ("split", spl)):
        e_y = max(float((y.double().cpu() - (p.clamp_min(0) if relu else p)).abs().max()) / max(1.0, float(p.abs().max())) for y, p in zip(ys, pre))
        masks = [(y.cpu() > 0) for y in ys] if relu else [torch.ones_like(p, dtype=torch.bool) for p in pre]       # each run against float64 under ITS OWN ReLU decisions
        gs = [t.double() * m for t, m in zip(dys, masks)]
        e_dx = max(float((o.double().cpu() - r).abs().max()) / max(1.0, float(r.abs().max()))
                   for o, r in zip(dx, [F.conv_transpose2d(t, wt.double(), None, padding=1) for t in gs]))
        w_ref = sum(torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), t, padding=1) for x, t in zip(xs, gs))
        e_dw = float((dw.double().cpu() - w_ref).abs().max()) / max(1.0, float(w_ref.abs().max()))
        out[tag] = (e_y, e_dx, e_dw)
    for en, es, bound in zip(out["native"], out["split"], (2e-5, 2e-5, 1e-4)):
        assert es < bound and es <= 1.5 * en + 2e-7, (name, out)


def test_conv3x3_f32_autograd_and_argument_checks(ops):
    """ops.conv3x3 (what VGGExtractor calls) under autograd against torch's conv2d + relu on the device, with the reference's own mask
    tolerance handled by a bias that keeps pre-activations away from zero; and the entry points refuse what the stage is not built for."""
    import torch.nn.functional as F
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 128, 64, 80, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(256, 128, 3, 3, generator=g) * 0.03).to(DEV).requires_grad_(True)
    b = (torch.randn(256, generator=g) * 0.1).to(DEV).requires_grad_(True)
    dy = torch.randn(1, 256, 64, 80, generator=g).to(DEV)
    ref = torch.relu(F.conv2d(x, w, b, padding=1))
    keep = ((ref > 1e-4) | (F.conv2d(x, w, b, padding=1) < -1e-4)).float()                       # gradient only where the sign is beyond rounding
    (ref * dy * keep).sum().backward()
    want = [t.grad.clone() for t in (x, w, b)]
    for t in (x, w, b):
        t.grad = None
    got_y = ops.conv3x3(x, w, b, relu=True)
    (got_y * dy * keep).sum().backward()
    assert float((got_y - ref).abs().max()) < 2e-5 * float(ref.abs().max())
    for a, c in zip([x.grad, w.grad, b.grad], want):
        assert float((a - c).abs().max()) < 1e-4 * max(1.0, float(c.abs().max()))
    assert ops.conv3x3_supported(x, w) and not ops.conv3x3_supported(x.half(), w) and not ops.conv3x3_supported(x[:, :, :8, :8], w)
    w32 = torch.zeros(128, 32, 3, 3, device=DEV, requires_grad=True)
    x32 = torch.zeros(1, 32, 256, 256, device=DEV)
    assert not ops.conv3x3_supported(x32, w32)                                                   # training needs Cin % 64 == 0
    with torch.no_grad():
        assert ops.conv3x3_supported(x32, w32)                                                   # forward only: Cin % 32 == 0
    with pytest.raises(FrcnnError):
        ops.conv3x3_wgrad([x32], [torch.zeros(1, 128, 256, 256, device=DEV)])
    with pytest.raises(FrcnnError):
        ops.conv3x3_fwd([x32], torch.zeros(32, 32, 3, 3, device=DEV))                            # Cout = 32
    big = torch.empty(1, 64, 1024, 2048, device=DEV)                                             # 36 x 1024 GEMM tiles: past the control block's ticket words
    assert not ops.conv3x3_supported(big, torch.zeros(64, 64, 3, 3, device=DEV, requires_grad=True))      # -> the caller keeps torch's convolution


@pytest.mark.parametrize("Cin,Cout,H,W", [(128, 128, 96, 132), (64, 128, 75, 125), (64, 64, 150, 250), (64, 64, 600, 1000), (128, 128, 300, 500)],
                         ids=["even", "odd_rows_cols", "narrow", "vgg_conv1_2_full_with_pool", "vgg_conv2_2_full_with_pool"])
def test_conv3x3_f32_fused_relu_maxpool(ops, Cin, Cout, H, W):
    """conv3x3(..., relu=True, pool=True) = Conv2d + ReLU + MaxPool2d(2, 2) of vgg16.features in one stage call: the pooled output and the
    words of the 2 x 2 windows come out of the output transform (the full-resolution activations are never written), and the gradient
    calls rebuild max_pool2d's + the ReLU's backward from the pooled gradient and the words while staging.  Checked (a) against float64
    (pooled values; gradients with the window selection decoded from the DEVICE words, which must agree with float64's own choice except
    where the two largest values of a window are within rounding) and (b) bit for bit against the unfused form of the same stage followed
    by torch's max_pool2d, forward and all gradients."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(H + Cin)
    x = torch.randn(1, Cin, H, W, generator=g)
    wt = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.2
    Hp, Wp = H // 2, W // 2
    dp = torch.randn(1, Cout, Hp, Wp, generator=g)
    xd, wd, bd, dpd = x.to(DEV), wt.to(DEV), b.to(DEV), dp.to(DEV)
    assert ops.conv3x3_pool_supported(xd)
    (yp,), xt, bits = ops.conv3x3_fwd([xd], wd, bd, True, keep_transformed=True, want_bits=True, pool=True)
    pre = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    act = pre.clamp_min(0)
    ref_p = F.max_pool2d(act, 2, 2)
    assert tuple(yp.shape) == (1, Cout, Hp, Wp)
    assert float((yp.double().cpu() - ref_p).abs().max()) < 2e-5 * max(1.0, float(pre.abs().max()))
    # decode the words: tile (ty, tx) of 4 x 4, window k = wi * 2 + wj: bits 3k .. 3k + 1 = position of the maximum, bit 3k + 2 = maximum > 0
    th, tw = (H + 3) // 4, (W + 3) // 4
    words = bits.cpu().view(Cout, -1)[:, :th * tw].to(torch.int32).bitwise_and(0xFFFF).view(Cout, th, tw)
    sel = torch.zeros(Cout, 4 * th, 4 * tw, dtype=torch.float64)
    for k in range(4):
        w3 = (words >> (3 * k)) & 7
        for pos in range(4):
            hit = (w3 == (4 | pos)).double()
            sel[:, (k // 2) * 2 + pos // 2::4, (k % 2) * 2 + pos % 2::4] = hit
    sel = sel[:, :H, :W]
    up = torch.zeros(1, Cout, H, W, dtype=torch.float64)
    up[:, :, :2 * Hp, :2 * Wp] = dp.double().repeat_interleave(2, 2).repeat_interleave(2, 3)
    gfull = up * sel                                                       # max_pool2d backward + ReLU backward with the device's selection
    # the device's selection = float64's own, except where a window's two largest activations are within rounding of each other (or of zero)
    _, idx = F.max_pool2d(act, 2, 2, return_indices=True)
    sel64 = torch.zeros(Cout, H * W, dtype=torch.float64).scatter_(1, idx.view(Cout, -1), (ref_p > 0).double().view(Cout, -1)).view(Cout, H, W)
    differ = (sel64 != sel)
    if int(differ.sum()):
        win = act[0, :, :2 * Hp, :2 * Wp].reshape(Cout, Hp, 2, Wp, 2).permute(0, 1, 3, 2, 4).reshape(Cout, Hp, Wp, 4)
        top2 = win.topk(2, dim=-1).values
        gap = torch.minimum(top2[..., 0] - top2[..., 1], top2[..., 0])          # distance to the runner-up, or to zero
        bad = differ[:, :2 * Hp, :2 * Wp].reshape(Cout, Hp, 2, Wp, 2).permute(0, 1, 3, 2, 4).reshape(Cout, Hp, Wp, 4).any(-1)
        assert float(gap[bad].max()) < 1e-5 and int(bad.sum()) < 1e-4 * bad.numel() + 4
    dx = ops.conv3x3_bwd_data([dpd], wd, bits, pooled_from=[(H, W)])[0]
    dx_ref = F.conv_transpose2d(gfull, wt.double(), None, padding=1)
    assert tuple(dx.shape) == (1, Cin, H, W)
    assert float((dx.double().cpu() - dx_ref).abs().max()) < 2e-5 * max(1.0, float(dx_ref.abs().max()))
    dw, db = ops.conv3x3_wgrad([xd], [dpd], bits, want_bias=True, x_transformed=xt, pooled=True)
    dyt = ops.conv3x3_dy_buffer([(H, W)], Cout, DEV)                         # the same with the pooled gradient staged once for both consumers
    dx_s = ops.conv3x3_bwd_data([dpd], wd, bits, pooled_from=[(H, W)], dy_transformed=dyt, want_bias_partials=True)[0]
    dw_s, db_s = ops.conv3x3_wgrad([xd], [dpd], bits, want_bias=True, x_transformed=xt, pooled=True, dy_transformed=dyt)
    assert torch.equal(dx, dx_s) and torch.equal(dw, dw_s) and torch.equal(db, db_s)
    w_ref = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), gfull, padding=1)
    assert float((dw.double().cpu() - w_ref).abs().max()) < 1e-4 * max(1.0, float(w_ref.abs().max()))
    assert float((db.double().cpu() - gfull.sum(dim=(0, 2, 3))).abs().max()) < 1e-4 * max(1.0, float(gfull.sum(dim=(0, 2, 3)).abs().max()))
    # (b) bit for bit against the unfused stage + torch's max_pool2d under autograd
    outs = []
    for fused in (True, False):
        xr, wr, br = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
        y = ops.conv3x3(xr, wr, br, relu=True, pool=True) if fused else F.max_pool2d(ops.conv3x3(xr, wr, br, relu=True), 2, 2)
        y.backward(dpd)
        outs.append((y.detach(), xr.grad, wr.grad, br.grad))
    for a_, c_ in zip(*outs):
        assert torch.equal(a_, c_)
    small = torch.zeros(1, 128, 12, 20, device=DEV)
    assert not ops.conv3x3_pool_supported(small)                            # 15 4 x 4 tiles would be padded to 64: the 2 x 2 tile, no fused pool
    with pytest.raises(Exception):
        ops.conv3x3_fwd([small], torch.zeros(128, 128, 3, 3, device=DEV), None, True, pool=True)
    # ... and so do the gradient calls (a stray `if` used to let a pooled gradient on the 2 x 2 tile through to an H x W staging of a half-size buffer)
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    w128 = torch.zeros(128, 128, 3, 3, device=DEV)
    _, _, bits_small = ops.conv3x3_fwd([small], w128, None, True, want_bits=True)
    with pytest.raises(FrcnnError):
        ops.conv3x3_bwd_data([torch.zeros(1, 128, 6, 10, device=DEV)], w128, bits_small, pooled_from=[(12, 20)])
    with pytest.raises(FrcnnError):
        ops.conv3x3_wgrad([small], [torch.zeros(1, 128, 6, 10, device=DEV)], bits_small, pooled=True)


@pytest.mark.parametrize("Cout,H,W", [(64, 75, 130), (32, 9, 700), (80, 33, 257), (64, 600, 1000), (64, 129, 20), (64, 7, 256), (48, 5, 512), (64, 1, 1)],
                         ids=["vgg_like", "wide", "two_words", "vgg_conv1_1_full", "tall_short_last_block", "one_forward_block_wide", "two_forward_blocks_wide", "one_pixel"])
def test_conv3x3_c3_first_convolution(ops, Cout, H, W):
    """frcnn_conv3x3_c3_fwd / _wgrad: `vgg16.features[0]` + `[1]` (Conv2d(3, 64, 3, padding=1) + ReLU) and their backward -- weight and bias
    gradient, the ReLU's backward from the forward's sign words -- against float64 (mask from the device output) and, through
    ops.conv3x3_c3 under autograd, against torch's own conv2d + relu on the device; bit-reproducible.
    The weight gradient puts several image rows in a block only where H x (groups of 32 channels) exceeds the CU count (frcnn_conv3x3_c3_wgrad):
    H = 600 takes five rows, which divide it; H = 129 with 64 channels takes two on 256 CUs and leaves ONE row to the last block.  W = 256 and 512 are
    the forward's block width exactly (no partial block), 1 x 1 is a map that is all border."""
    import torch.nn.functional as F
    if (Cout, H, W) == (64, 129, 20):
        cus = torch.cuda.get_device_properties(DEV).multi_processor_count         # hipDeviceAttributeMultiprocessorCount, what the launch asks
        rows = max(1, min((150 * 1024) // (12 * (W + 2)) - 2, -(-H * ((Cout + 31) // 32) // cus)))
        print("\n[c3 tall] %d CUs: %d rows per block, %d blocks, %d rows in the last" % (cus, rows, -(-H // rows), H - (-(-H // rows) - 1) * rows))
        assert cus != 256 or (rows == 2 and H % rows == 1)
    g = torch.Generator().manual_seed(Cout + W)
    x = torch.randn(1, 3, H, W, generator=g)
    wt = torch.randn(Cout, 3, 3, 3, generator=g) * 0.3
    b = torch.randn(Cout, generator=g) * 0.2
    dy = torch.randn(1, Cout, H, W, generator=g)
    xd, wd, bd, dyd = x.to(DEV), wt.to(DEV), b.to(DEV), dy.to(DEV)
    y, bits = ops.conv3x3_c3_fwd(xd, wd, bd, True, want_bits=True)
    pre = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    assert float((y.double().cpu() - pre.clamp_min(0)).abs().max()) < 1e-5 * max(1.0, float(pre.abs().max()))
    assert torch.equal(y, ops.conv3x3_c3_fwd(xd, wd, bd, True))
    lin = ops.conv3x3_c3_fwd(xd, wd, None, False)
    assert float((lin.double().cpu() - F.conv2d(x.double(), wt.double(), None, padding=1)).abs().max()) < 1e-5 * max(1.0, float(pre.abs().max()))
    mask = (y.cpu() > 0)
    flips = mask != (pre > 0)
    assert int(flips.sum()) == 0 or float(pre[flips].abs().max()) < 1e-5
    gm = dy.double() * mask
    dw, db = ops.conv3x3_c3_wgrad(xd, dyd, bits)
    w_ref = torch.nn.grad.conv2d_weight(x.double(), (Cout, 3, 3, 3), gm, padding=1)
    assert float((dw.double().cpu() - w_ref).abs().max()) < 1e-4 * max(1.0, float(w_ref.abs().max()))
    assert float((db.double().cpu() - gm.sum(dim=(0, 2, 3))).abs().max()) < 1e-4 * max(1.0, float(gm.sum(dim=(0, 2, 3)).abs().max()))
    dw2, db2 = ops.conv3x3_c3_wgrad(xd, dyd, bits)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    dw0, _ = ops.conv3x3_c3_wgrad(xd, dyd, None)                                  # no ReLU: the plain weight gradient
    w0 = torch.nn.grad.conv2d_weight(x.double(), (Cout, 3, 3, 3), dy.double(), padding=1)
    assert float((dw0.double().cpu() - w0).abs().max()) < 1e-4 * max(1.0, float(w0.abs().max()))
    if Cout % 16 == 0:
        wr, br = wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
        assert ops.conv3x3_c3_supported(xd, wr)
        out = ops.conv3x3_c3(xd, wr, br, relu=True)
        out.backward(dyd)
        assert torch.equal(out.detach(), y) and torch.equal(wr.grad, dw) and torch.equal(br.grad, db)


def test_fused_relu_keeps_a_nan_like_torch_relu(ops):
    """the ReLUs fused into the conv stage's output transform (plain and with the 2 x 2 max-pool) and into the first convolution must
    propagate a NaN as torch.relu / clamp_min / max_pool2d do -- fmaxf(NaN, 0) returns 0 and would hide a diverged activation.  The first
    convolution is a direct sum: its NaN set equals torch's.  The Winograd stage transforms 6 x 6 patches, so a NaN input reaches every output
    of the tiles whose patch holds it: a superset of torch's 3 x 3 neighbourhood, never a subset."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    x3 = torch.randn(1, 3, 40, 70, generator=g).to(DEV)
    x3[0, 1, 17, 33] = float("nan")
    w3 = (torch.randn(64, 3, 3, 3, generator=g) * 0.3).to(DEV)
    b3 = torch.randn(64, generator=g).to(DEV)
    y = ops.conv3x3_c3_fwd(x3, w3, b3, True)
    ref = torch.relu(F.conv2d(x3, w3, b3, padding=1))
    assert int(torch.isnan(ref).sum()) == 64 * 9 and torch.equal(torch.isnan(y), torch.isnan(ref))
    x = torch.randn(1, 128, 96, 132, generator=g).to(DEV)
    x[0, 5, 41, 77] = float("nan")
    w = (torch.randn(128, 128, 3, 3, generator=g) * 0.03).to(DEV)
    b = torch.randn(128, generator=g).to(DEV)
    ref = torch.relu(F.conv2d(x, w, b, padding=1))
    y = ops.conv3x3_fwd([x], w, b, True)[0]
    nan_ref, nan_y = torch.isnan(ref), torch.isnan(y)
    assert int(nan_ref.sum()) == 128 * 9 and bool((nan_y | ~nan_ref).all()) and int(nan_y.sum()) <= 128 * 64
    yp = ops.conv3x3_fwd([x], w, b, True, pool=True)[0]
    nan_p = torch.isnan(F.max_pool2d(ref, 2, 2))
    assert int(nan_p.sum()) > 0 and bool((torch.isnan(yp) | ~nan_p).all())
    small = torch.randn(1, 128, 12, 20, generator=g).to(DEV)               # the 2 x 2 tile's output transform
    small[0, 0, 6, 9] = float("nan")
    ys = ops.conv3x3_fwd([small], w, b, True)[0]
    nan_s = torch.isnan(torch.relu(F.conv2d(small, w, b, padding=1)))
    assert bool((torch.isnan(ys) | ~nan_s).all())


@pytest.mark.parametrize("M,N,K", [(128, 512, 16800), (256, 256, 67200), (64, 192, 96), (512, 128, 4224)])
def test_gemm_nt_and_the_1x1_convolution_weight_gradient(ops, M, N, K):
    """frcnn_gemm_nt_f32 (O = A . B^T, both operands k-contiguous, fixed summation order) against float64, bit-reproducible; and ops.conv1x1 -- torch's
    forward / input gradient / bias gradient with dW on that GEMM -- against torch's own conv2d under autograd."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(M + K)
    a = torch.randn(M, K, generator=g)
    b = torch.randn(N, K, generator=g)
    out = ops.gemm_nt(a.to(DEV), b.to(DEV))
    ref = a.double() @ b.double().t()
    assert float((out.double().cpu() - ref).abs().max()) < 1e-5 * K ** 0.5 * 4
    assert torch.equal(out, ops.gemm_nt(a.to(DEV), b.to(DEV)))
    if K % 168 == 0:                                                          # as a convolution: [1, N, h, 168] -> [1, M, h, 168]
        h = K // 168
        x = b.reshape(1, N, h, 168).to(DEV).requires_grad_(True)
        w = (torch.randn(M, N, 1, 1, generator=g) * 0.05).to(DEV).requires_grad_(True)
        bias = torch.randn(M, generator=g).to(DEV).requires_grad_(True)
        dy = a.reshape(1, M, h, 168).to(DEV)
        assert ops.conv1x1_supported(x, w)
        y = ops.conv1x1(x, w, bias)
        y.backward(dy)
        got = [y.detach(), x.grad.clone(), w.grad.clone(), bias.grad.clone()]
        for t in (x, w, bias):
            t.grad = None
        y2 = F.conv2d(x, w, bias)
        y2.backward(dy)
        assert torch.equal(got[0], y2.detach()) and torch.equal(got[1], x.grad) and torch.equal(got[3], bias.grad)
        assert float((got[2] - w.grad).abs().max()) < 1e-4 * max(1.0, float(w.grad.abs().max()))
    with pytest.raises(Exception):
        ops.gemm_nt(torch.zeros(64, 40, device=DEV), torch.zeros(64, 40, device=DEV))      # K % 32 != 0


@pytest.mark.parametrize("with_res,relu", [(False, True), (True, True), (False, False), (True, False)])
def test_affine_act_is_the_torch_form_bit_for_bit(ops, with_res, relu):
    """frcnn_affine_act_fwd / _bwd: FrozenBatchNorm2d (+ residual) (+ ReLU) of torchvision's Bottleneck.forward in one pass each way -- the torch
    form's operations in its order, so values and gradients are bit-identical to `relu(x * scale + shift + res)` under autograd."""
    g = torch.Generator().manual_seed(5 + with_res * 2 + relu)
    C_, H, W = 96, 37, 53                                                       # an odd plane size: tails of the 1024-element pieces
    x = torch.randn(1, C_, H, W, generator=g).to(DEV).requires_grad_(True)
    r = torch.randn(1, C_, H, W, generator=g).to(DEV).requires_grad_(True) if with_res else None
    scale = (torch.rand(C_, generator=g) + 0.5).to(DEV)
    shift = torch.randn(C_, generator=g).to(DEV)
    dy = torch.randn(1, C_, H, W, generator=g).to(DEV)
    ref = x * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)
    if with_res:
        ref = ref + r
    if relu:
        ref = torch.relu(ref)
    ref.backward(dy)
    want = [x.grad.clone()] + ([r.grad.clone()] if with_res else [])
    x.grad = None
    if with_res:
        r.grad = None
    out = ops.affine_act(x, scale, shift, r, relu)
    out.backward(dy)
    assert torch.equal(out, ref)
    for a_, c_ in zip([x.grad] + ([r.grad] if with_res else []), want):
        assert torch.equal(a_, c_)
    assert ops.affine_act_supported(x) and not ops.affine_act_supported(x.half())
    # a NaN activation stays a NaN through the fused ReLU, as through torch.relu (fmaxf(NaN, 0) would have returned 0: ADVICE r4)
    xn = x.detach().clone()
    xn[0, 3, 5, 7] = float("nan")
    xn[0, 4, 0, 0] = float("-inf")
    out_n = ops.affine_act(xn, scale, shift, r.detach() if with_res else None, relu)
    ref_n = xn * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)
    if with_res:
        ref_n = ref_n + r.detach()
    if relu:
        ref_n = torch.relu(ref_n)
    assert bool(torch.isnan(out_n[0, 3, 5, 7])) and torch.equal(torch.isnan(out_n), torch.isnan(ref_n))
    assert torch.equal(torch.nan_to_num(out_n, nan=7.0), torch.nan_to_num(ref_n, nan=7.0))


def test_conv3x3_bf16_c256_vs_torch(ops):
    """ops.conv3x3_bf16_c256 (BASELINE configs[4]: the FPN's 256 -> 256 output convolutions under bf16 autocast, from the RPN head's bf16 MFMA kernels --
    the forward is the data-gradient kernel on the transposed, flipped weight): forward, input gradient and weight gradient against a float64 convolution
    of the same bf16-rounded operands (fp32 accumulate, one bf16 rounding of the outputs: 1e-2 of the scale; the weight gradient stays fp32: 2e-3)."""
    g = torch.Generator().manual_seed(3)
    H, W = 100, 168
    x = (torch.randn(1, 256, H, W, generator=g) * 0.5).to(DEV).bfloat16().requires_grad_(True)
    w = (torch.randn(256, 256, 3, 3, generator=g) * 0.03).to(DEV).requires_grad_(True)
    b = torch.randn(256, generator=g).to(DEV).requires_grad_(True)
    dy = torch.randn(1, 256, H, W, generator=g).to(DEV).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert ops.conv3x3_bf16_c256_supported(x, w)
        y = ops.conv3x3_bf16_c256(x, w, b)
    assert y.dtype == torch.bfloat16
    y.backward(dy)
    x64 = x.detach().double().requires_grad_(True)
    w64 = w.detach().bfloat16().double().requires_grad_(True)             # the kernels round the weight to bf16 when they pack it
    b64 = b.detach().double().requires_grad_(True)
    y64 = torch.nn.functional.conv2d(x64, w64, b64.bfloat16().double() if False else b64, padding=1)
    y64.backward(dy.double())
    rel = lambda a, c: float((a.double() - c).abs().max() / c.abs().max())      # noqa: E731
    assert rel(y, y64) < 1e-2, rel(y, y64)
    assert rel(x.grad, x64.grad) < 1e-2, rel(x.grad, x64.grad)
    assert w.grad.dtype == torch.float32 and rel(w.grad, w64.grad) < 2e-3, rel(w.grad, w64.grad)
    assert rel(b.grad, b64.grad) < 1e-2
    assert not ops.conv3x3_bf16_c256_supported(x.detach()[:, :, :50, :84], w)   # small maps stay with the vendor convolution


@pytest.mark.parametrize("form", ["inner", "stream", "stream_res_twin", "f32_res_twin"])
def test_affine_act_mixed_is_the_autocast_torch_form(ops, form):
    """frcnn_affine_act_fwd_mixed / _bwd_mixed (BASELINE configs[4], bf16 autocast; csrc/affine.hip): the frozen norm (+ residual) (+ ReLU) with bf16 on either
    side of the fp32 arithmetic.  Against the torch expressions the model ran under autocast before: an INNER norm = relu(addcmul(shift_bf16, x_bf16, scale_bf16))
    up to the rounding of scale / shift to bf16 it no longer does (compared with the fp32-parameter form rounded once: equal bit for bit); the STREAM form =
    relu(x_bf16 * scale + shift [+ res]) in fp32: bit for bit, and its bf16 twin = that value's .bfloat16(); gradients: dx = (mask * (g + g_twin)) * scale rounded
    to x's dtype, dres = mask * (g + g_twin): bit for bit with autograd on the torch form."""
    g = torch.Generator().manual_seed(11)
    C_, H, W = 64, 29, 45
    xb = (form != "f32_res_twin")
    x = torch.randn(1, C_, H, W, generator=g).to(DEV)
    x = (x.bfloat16() if xb else x).requires_grad_(True)
    with_res, twin, inner = form.endswith("res_twin"), form.endswith("twin"), form == "inner"
    r = torch.randn(1, C_, H, W, generator=g).to(DEV).requires_grad_(True) if with_res else None
    scale = (torch.rand(C_, generator=g) + 0.5).to(DEV)
    shift = torch.randn(C_, generator=g).to(DEV)
    ref32 = x.float() * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)
    if with_res:
        ref32 = ref32 + r
    ref32 = torch.relu(ref32)
    ref = ref32.bfloat16() if inner else ref32
    ref_twin = ref32.bfloat16() if twin else None
    dy = torch.randn(1, C_, H, W, generator=g).to(DEV)
    dy = dy.bfloat16() if inner else dy
    dt = torch.randn(1, C_, H, W, generator=g).to(DEV).bfloat16() if twin else None
    torch.autograd.backward([ref] + ([ref_twin] if twin else []), [dy] + ([dt] if twin else []))
    want = [x.grad.clone()] + ([r.grad.clone()] if with_res else [])
    x.grad = None
    if with_res:
        r.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert ops.affine_act_mixed_supported(x)
        out = ops.affine_act_mixed(x, scale, shift, r, relu=True, out_bf16=inner, twin=twin)
    y, yt = out if twin else (out, None)
    assert y.dtype == (torch.bfloat16 if inner else torch.float32) and torch.equal(y, ref)
    if twin:
        assert yt.dtype == torch.bfloat16 and torch.equal(yt, ref_twin)
    torch.autograd.backward([y] + ([yt] if twin else []), [dy] + ([dt] if twin else []))
    assert x.grad.dtype == x.dtype
    # the torch form rounds the twin's gradient path separately (bf16 -> fp32 is exact; the SUM g + g_twin is formed in fp32 in both): bit for bit,
    # except that autograd's own accumulation order (g_twin + g vs g + g_twin) is commutative anyway
    for a_, c_ in zip([x.grad] + ([r.grad] if with_res else []), want):
        assert torch.equal(a_, c_)
    assert not ops.affine_act_mixed_supported(x.detach())                        # outside autocast the fp32 op (or torch) serves


@pytest.mark.parametrize("m", ["2", "4"])
def test_conv3x3_f32_forced_tile_size_in_a_child_process(m):
    """The stage picks its tile by cost (4 x 4 wherever 36 planes x its padded tile total is 15 % below 16 x the 2 x 2 total); FRCNN_WINO_M (read once per process) forces one.  A child process
    runs a large map with the small tile and small / odd maps with the large one (what the default choice never does) against float64: forward with
    bias + ReLU, masked data gradient, weight + bias gradient; 2e-5 of the scale for m = 2, 5e-5 for m = 4 (its transform constants span 1/24 .. 8)."""
    import subprocess
    code = r"""
import os, torch, torch.nn.functional as F
from faster_rcnn_pytorch_amd import ops
dev = "cuda:0"
tol = 2e-5 if os.environ["FRCNN_WINO_M"] == "2" else 5e-5
for Cin, Cout, shapes in ((128, 256, [(96, 130)]), (256, 128, [(9, 14), (30, 5), (1, 1), (4, 4)]), (128, 128, [(37, 62)])):
    g = torch.Generator().manual_seed(Cin + len(shapes))
    xs = [torch.randn(1, Cin, h, w, generator=g) for h, w in shapes]
    wt = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.2
    dys = [torch.randn(1, Cout, h, w, generator=g) for h, w in shapes]
    xd, dyd, wd, bd = [x.to(dev) for x in xs], [t.to(dev) for t in dys], wt.to(dev), b.to(dev)
    ys, _, bits = ops.conv3x3_fwd(xd, wd, bd, True, want_bits=True)
    pre = [F.conv2d(x.double(), wt.double(), b.double(), padding=1) for x in xs]
    for y, p in zip(ys, pre):
        assert float((y.double().cpu() - p.clamp_min(0)).abs().max()) < tol * max(1.0, float(p.abs().max()))
    gs = [t.double() * (y.cpu() > 0) for t, y in zip(dys, ys)]
    dx = ops.conv3x3_bwd_data(dyd, wd, bits)
    for o, t in zip(dx, gs):
        r = F.conv_transpose2d(t, wt.double(), None, padding=1)
        assert float((o.double().cpu() - r).abs().max()) < tol * max(1.0, float(r.abs().max()))
    dw, db = ops.conv3x3_wgrad(xd, dyd, bits, want_bias=True)
    w_ref = sum(torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), t, padding=1) for x, t in zip(xs, gs))
    b_ref = sum(t.sum(dim=(0, 2, 3)) for t in gs)
    assert float((dw.double().cpu() - w_ref).abs().max()) < 1e-4 * max(1.0, float(w_ref.abs().max()))
    assert float((db.double().cpu() - b_ref).abs().max()) < 1e-4 * max(1.0, float(b_ref.abs().max()))
print("forced tile OK")
"""
    e = dict(os.environ, FRCNN_WINO_M=m, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "forced tile OK" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------ RoIAlign forward dispatch order (round 4)
def test_roi_scale_order_and_ordered_forward_are_bit_identical(ops):
    """frcnn_roi_scale_order replaces the `roi * (w, h, w, h)` launch of FastRCNNHead.forward (models/new_model.py:136-140) and also hands
    out the order in which the pooling's workgroups are dispatched (largest footprint first).  The scaled boxes must be torch's own
    products bit for bit, `order` a permutation along which the cost keys do not increase (ties by index), and the pooled output must
    not depend on the order: bit-identical to the unordered call and to the oracle-checked path, for the library's order, a random
    permutation and the reversed order."""
    rng = np.random.RandomState(41)
    H, W = 800, 1344
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42)]
    scales = (0.25, 0.125, 0.0625, 0.03125)
    R = 512
    b = rand_boxes(rng, R, 0.01, 0.9)                                          # normalised boxes of every size: all four levels, 1-4 staging passes
    b[:7] = np.array([[0, 0, 1, 1], [0.1, 0.1, 0.1001, 0.1001], [0, 0, 1, 0.02], [0.3, 0, 0.31, 1], [0.5, 0.5, 0.5, 0.5], [0, 0, 0.99, 0.99], [0.2, 0.2, 0.8, 0.8]], np.float32)
    mul = np.array([W, H, W, H], np.float32)
    tb = T(b)
    scaled, order, cost = ops.roi_scale_order(tb, mul, shapes, scales, want_cost=True)
    assert torch.equal(scaled, tb * T(mul))                                     # the same fp32 products as the elementwise launch it replaces
    o = order.cpu().numpy().astype(np.int64)
    c = cost.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert sorted(o.tolist()) == list(range(R))
    ck = c[o]
    assert (np.diff(ck) <= 0).all()
    assert all(o[i] < o[i + 1] for i in range(R - 1) if ck[i] == ck[i + 1])      # ties by index
    passes, fp = ck >> 20, ck & 0xFFFFF
    assert passes.max() > passes.min() and passes.min() >= 1                     # the test frame really mixes short and long workgroups
    # footprint of the key = the oracle-independent geometry: pixels of the level-scaled box, give or take the sampling border
    lv = ops.roi_level_map(scaled).cpu().numpy()
    sc = np.asarray(scales)[lv]
    approx = (np.clip((b[:, 2] - b[:, 0]) * W * sc, 1, None) + 2) * (np.clip((b[:, 3] - b[:, 1]) * H * sc, 1, None) + 2)
    rel = np.abs(np.log((c & 0xFFFFF)[: R].clip(1) / approx.clip(1)))
    assert np.median(rel) < 0.7
    feats = [torch.randn(1, 256, h, w, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) for h, w in shapes]
    base = ops.ms_roi_align(feats, scaled, 7, 2, scales)
    for perm in (order, T(rng.permutation(R).astype(np.int32)), torch.flip(order, [0]).contiguous()):
        got = ops.ms_roi_align(feats, scaled, 7, 2, scales, order=perm)
        assert torch.equal(got, base)
    ref, _ = orc.ms_roi_align([f[0].cpu().numpy() for f in feats], scaled.cpu().numpy(), scales=scales)
    assert np.abs(base.cpu().numpy() - ref).max() < 1e-5


@pytest.mark.parametrize("name", ["vgg600x1000", "fpn_small"])
def test_rpn_conv3x3_f32_matches_the_references_cpu_path_golden(ops, golden, name):
    """north_star: tensors within 1e-4 of the reference's CPU path on identical inputs.  `inter_layer` on the CPU is torch's fp32
    conv2d + autograd (tests/golden/make_golden_rpn_conv.py restates the layer and its init: models/model.py:68-77); the committed
    fixture holds strided samples of its forward output and of both gradients; the inputs are regenerated from the seed and their
    sha256 checked."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mk_rpn_conv", os.path.join(ROOT, "tests", "golden", "make_golden_rpn_conv.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    g = golden("rpn_conv")
    C, shapes, w, feats, gouts = mk.inputs(name)
    if mk.sha([w] + feats + gouts) != str(g[name + "_inputs_sha256"]):
        pytest.skip("this torch build draws other random inputs than the one that made the fixture")
    wd, fd, gd = w.to(DEV), [f.to(DEV) for f in feats], [t.to(DEV) for t in gouts]
    outs = ops.rpn_conv3x3_fwd(fd, wd)
    dxs = ops.rpn_conv3x3_bwd_data(gd, wd)
    dw = ops.rpn_conv3x3_wgrad(fd, gd)

    def close(got, want):
        got = got.reshape(-1)[::mk.STRIDE].cpu().numpy()
        assert got.shape == want.shape
        assert np.abs(got - want).max() < 1e-4 * max(1.0, float(np.abs(want).max())), np.abs(got - want).max()
    for k in range(len(shapes)):
        close(outs[k], g["%s_out%d" % (name, k)])
        close(dxs[k], g["%s_dx%d" % (name, k)])
    close(dw, g[name + "_dw"])


def test_rpn_conv3x3_f32_direct_form_in_a_child_process():
    """Forward, data gradient and weight gradient run through the Winograd domain (four launches each); the direct kernels (K = 9 C
    stream-K kernel, + pack kernel for the data gradient; per-wave K-range weight gradient) stay in the library behind
    FRCNN_CONV_F32_DIRECT=1 (read once per process).  A child process runs it at the
    600x1000 shape, three small FPN levels and an odd shape against float64, like the default form above."""
    import subprocess
    code = r'''
import torch, torch.nn.functional as F
from faster_rcnn_pytorch_amd import ops, _lib
dev = "cuda:0"
for C, shapes in ((512, [(37, 62)]), (256, [(50, 84), (25, 42), (13, 21)]), (128, [(5, 7), (1, 1), (3, 130), (17, 2)])):
    g = torch.Generator().manual_seed(C)
    feats = [torch.randn(1, C, h, w, generator=g) for h, w in shapes]
    wt = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    gouts = [torch.randn(1, C, h, w, generator=g) for h, w in shapes]
    _lib.prof_reset(); _lib.prof_enable(True)
    out = ops.rpn_conv3x3_fwd([f.to(dev) for f in feats], wt.to(dev))
    dx = ops.rpn_conv3x3_bwd_data([t.to(dev) for t in gouts], wt.to(dev))
    dw = ops.rpn_conv3x3_wgrad([f.to(dev) for f in feats], [t.to(dev) for t in gouts])
    _lib.prof_enable(False)
    names = set(_lib.prof_report())
    assert {"rpn_conv3x3_f32_kernel", "rpn_conv_f32_pack_kernel", "rpn_conv3x3_f32_wgrad_kernel"} <= names and not any("wino" in n for n in names), names
    wref = sum(torch.nn.grad.conv2d_weight(f.double(), (C, C, 3, 3), t.double(), padding=1) for f, t in zip(feats, gouts))
    assert float((dw.double().cpu() - wref).abs().max()) < 1e-4 * max(1.0, float(wref.abs().max()))
    for o, f in zip(out, feats):
        r = F.conv2d(f.double(), wt.double(), None, padding=1)
        assert float((o.double().cpu() - r).abs().max()) < 2e-5 * max(1.0, float(r.abs().max()))
    for o, t in zip(dx, gouts):
        r = F.conv_transpose2d(t.double(), wt.double(), None, padding=1)
        assert float((o.double().cpu() - r).abs().max()) < 2e-5 * max(1.0, float(r.abs().max()))
print("direct form OK")
'''
    e = dict(os.environ, FRCNN_CONV_F32_DIRECT="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "direct form OK" in r.stdout, r.stdout + r.stderr


def test_conv3x3_f32_unfused_product_in_a_child_process(ops):
    """64 -> 64 channels on 4 x 4 tiles run the product and the output transform as ONE launch (rpn_wino_gemm_out64_kernel: the 36 products of a (channel, tile)
    stay in the accumulators); FRCNN_WINO_NO_FUSE=1 (read once per process) keeps the two launches.  Both forms against float64 -- forward with bias + ReLU and
    with the fused 2 x 2 max-pool, sign / window words, the masked data gradient -- on a map whose tile count is no multiple of 32 and whose last tile row and
    column are partial; and the two forms against each other within the rounding of their different summation orders."""
    import subprocess, sys, tempfile, os
    code = r"""
import sys, torch, torch.nn.functional as F
from faster_rcnn_pytorch_amd import ops
dev = "cuda:0"
g = torch.Generator().manual_seed(11)
H, W = 118, 203
x = torch.randn(1, 64, H, W, generator=g); wt = torch.randn(64, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5; b = torch.randn(64, generator=g) * 0.2
dy = torch.randn(1, 64, H, W, generator=g); dyp = torch.randn(1, 64, H // 2, W // 2, generator=g)
xd, wd, bd = x.to(dev), wt.to(dev), b.to(dev)
pre = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
ys, _, bits = ops.conv3x3_fwd([xd], wd, bd, True, want_bits=True)
assert float((ys[0].double().cpu() - pre.clamp_min(0)).abs().max()) < 5e-5 * float(pre.abs().max())
assert torch.equal(ys[0], ops.conv3x3_fwd([xd], wd, bd, True)[0])
dx = ops.conv3x3_bwd_data([dy.to(dev)], wd, bits)[0]
r = F.conv_transpose2d(dy.double() * (ys[0].cpu() > 0), wt.double(), None, padding=1)
assert float((dx.double().cpu() - r).abs().max()) < 5e-5 * float(r.abs().max())
yp, _, pw = ops.conv3x3_fwd([xd], wd, bd, True, want_bits=True, pool=True)
rp = F.max_pool2d(pre.clamp_min(0), 2, 2)
assert float((yp[0].double().cpu() - rp).abs().max()) < 5e-5 * float(pre.abs().max())
dxp = ops.conv3x3_bwd_data([dyp.to(dev)], wd, pw, pooled_from=[(H, W)])[0]
torch.save({"y": ys[0].cpu(), "dx": dx.cpu(), "yp": yp[0].cpu(), "dxp": dxp.cpu()}, sys.argv[1])
print("ok")
"""
    outs = []
    with tempfile.TemporaryDirectory() as td:
        for flag in ("0", "1"):
            path = os.path.join(td, "o%s.pt" % flag)
            env = dict(os.environ, FRCNN_WINO_NO_FUSE=flag)
            res = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300,
                                 cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            assert res.returncode == 0 and "ok" in res.stdout, res.stderr[-2000:]
            outs.append(torch.load(path))
    for k in ("y", "dx", "yp", "dxp"):
        a_, c_ = outs[0][k], outs[1][k]
        assert a_.shape == c_.shape and float((a_ - c_).abs().max()) < 2e-5 * max(1.0, float(c_.abs().max())), k

