"""CPU proof of tests/targets_ref.py before any kernel is looked at: on every seam case the exact restatement of the target makers
equals the C oracle (labels, counts, kept indices, classes, sampled RoIs and the exact target columns bit for bit; the logarithms
within the suite's bounds), the guard check_decidable() lets every case through, and every case holds the seam it is named for.
A few lattice-snapped versions of the random cases of tests/test_gpu_ops.py tie the restatement to the oracle on ordinary data
as well (the goldens tie the oracle to the reference project)."""
import numpy as np
import pytest

import targets_ref as tr
from oracle import oracle as orc
from oracle import philox_ref

RPN_NAMES = tr.rpn_case_names()
HEAD_NAMES = tr.head_case_names()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _close_or_same_special(got, want, tol):
    """finite entries within tol, non-finite ones identical"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    return np.array_equal(got[~fin], want[~fin], equal_nan=True) and (got[fin].size == 0 or np.abs(got[fin] - want[fin]).max() < tol)


def _rpn_vs_oracle(c, perms):
    r = tr.rpn_match(c)
    a, g = tr.to_f32(c.anchors), tr.to_f32(c.gt)
    pre_o, reg_o, counts_o = orc.rpn_targets(a, g, variant=c.variant)
    assert counts_o == (r.n_pos, r.n_neg), c.name
    assert np.array_equal(pre_o, r.pre), c.name
    assert np.array_equal(reg_o[:, :2].view(np.uint32), r.reg01.view(np.uint32)), c.name       # (bit patterns: NaN-safe)
    assert _close_or_same_special(reg_o[:, 2:], r.reg23, 1e-6), c.name
    for pp, pn in perms:
        assert np.array_equal(orc.rpn_targets(a, g, pp, pn, variant=c.variant)[0], tr.rpn_sample(c, pp, pn)), c.name


def _philox_rpn_perms(c, seed, offset):
    r = tr.rpn_match(c)
    return (philox_ref.sampling_perm(seed, offset, 1, np.nonzero(r.pre == 1)[0]), philox_ref.sampling_perm(seed, offset, 0, np.nonzero(r.pre == 0)[0]))


@pytest.mark.parametrize("name", RPN_NAMES)
def test_rpn_case_holds_its_seam_is_decidable_and_equals_the_oracle(name):
    c = tr.rpn_case(name)
    c.seam(c, tr.rpn_match(c))
    tr.check_decidable(c)                                  # a rejected case FAILS
    _rpn_vs_oracle(c, [tr.rpn_perms(c), _philox_rpn_perms(c, 11, 3)])


def _head_vs_oracle(c, perms):
    r = tr.head_match(c)
    rois, g = tr.to_f32(c.rois[:c.n_rois]), tr.to_f32(c.gt)
    assert orc.head_target_counts(rois, g, c.gt_label, c.variant) == (r.npc, r.nnc), c.name
    for pp, pn in perms:
        keep, cls, reg01, reg23, counts = tr.head_sample(c, pp, pn)
        cls_o, reg_o, rois_o, keep_o = orc.head_targets(rois, g, c.gt_label, pp, pn, c.variant, c.label_offset, c.max_pos, c.total)
        assert len(keep_o) == counts[2] and np.array_equal(keep_o, keep) and np.array_equal(cls_o, cls), c.name
        assert _same_bits(rois_o, tr.to_f32(r.cand[keep])), c.name
        assert _same_bits(reg_o[:, :2], reg01), c.name
        assert _close_or_same_special(reg_o[:, 2:], reg23, 1e-5), c.name


def _philox_head_perms(c, seed, offset):
    r = tr.head_match(c)
    return philox_ref.sampling_perm(seed, offset, 2, r.pos_list), philox_ref.sampling_perm(seed, offset, 3, r.neg_list)


@pytest.mark.parametrize("name", HEAD_NAMES)
def test_head_case_holds_its_seam_is_decidable_and_equals_the_oracle(name):
    c = tr.head_case(name)
    c.seam(c, tr.head_match(c))
    tr.check_decidable(c)
    _head_vs_oracle(c, [tr.head_perms(c, k) for k in ("identity", "reversed", "random")] + [_philox_head_perms(c, 5, 9)])


def test_the_case_lists_hold_every_seam_the_issue_names():
    assert tr.G_ROUNDS == [1, 63, 64, 65, 128, 129, 4096]
    assert tr.N_SEAMS == [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 24575, 24576, 24577]
    assert tr.HEAD_N_SEAMS == [1023, 1024, 1025, 2048, 2049, 4095, 4096]
    assert {"N%d-sampled-v%d" % (N, v) for N in (1023, 1024, 1025, 24575, 24576, 24577) for v in (0, 1)} <= set(RPN_NAMES)
    assert {(i, j) for i, j in tr.TIE_PAIRS} >= {(5, 6), (70, 134), (255, 256), (1023, 1024), (0, tr.TIE_N - 1)}
    for v in (0, 1):
        for fam in ("tie-v%d-straight", "tie-v%d-swapped", "tie-symmetric-v%d", "thresholds-v%d", "lonely-gt-v%d", "zero-area-gt-v%d", "zero-area-anchor-v%d"):
            assert fam % v in RPN_NAMES
        assert {"quota-v%d-pos%d-neg%+d" % (v, p, d) for p in (127, 128, 129) for d in (-1, 0, 1)} <= set(RPN_NAMES)
        assert {"quota-v%d-pos%+d-neg%+d" % (v, p, d) for p in (-1, 0, 1) for d in (-1, 0, 1)} <= set(HEAD_NAMES)
        for fam in ("device-count-v%d", "thresholds-v%d", "argmax-ties-v%d", "rows1024-v%d"):
            assert fam % v in HEAD_NAMES
    assert len(set(RPN_NAMES)) == len(RPN_NAMES) and len(set(HEAD_NAMES)) == len(HEAD_NAMES)


def test_fp32_division_returns_the_threshold_constants_on_exact_hits():
    """the guard's second clause, for the pairs the cases use and for every lattice scaling of 7/10, 3/10 and 1/2 up to the image's area"""
    for num, den, t in ((7, 10, 0.7), (3, 10, 0.3), (1, 2, 0.5)):
        k = np.arange(1, 2048 // den + 1, dtype=np.float32)
        assert (np.float32(num) * k / (np.float32(den) * k) == np.float32(t)).all()
        assert ((np.float32(num) * k / 1024) / (np.float32(den) * k / 1024) == np.float32(t)).all()


def test_f32_of_is_the_correctly_rounded_fp32_value():
    from fractions import Fraction
    rng = np.random.RandomState(0)
    for _ in range(2000):
        p, q = int(rng.randint(-4000, 4000)), int(rng.randint(1, 4000))
        assert np.float32(tr.f32_of(Fraction(p, q))) == np.float32(p) / np.float32(q)          # IEEE division of two exact operands
    assert tr.f32_of(Fraction((1 << 24) + 1, 1 << 24)) == 1.0 and tr.f32_of(Fraction((1 << 24) + 3, 1 << 24)) == 1.0 + 2.0 ** -22   # ties to even


def _snap(boxes):
    """fp32 boxes in [0, 1] -> the lattice, degenerate results widened by one step"""
    b = np.rint(np.asarray(boxes, np.float64) * tr.LAT).astype(np.int64)
    b[:, 2] = np.maximum(b[:, 2], b[:, 0] + 1)
    b[:, 3] = np.maximum(b[:, 3], b[:, 1] + 1)
    return b


def _rand_gt(rng, G):
    c = rng.rand(G, 2) * 0.7 + 0.15
    wh = rng.rand(G, 2) * 0.52 + 0.08
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1)


def _rand_boxes(rng, n, lo, hi):
    c = rng.rand(n, 2) * 0.8 + 0.1
    wh = rng.rand(n, 2) * (hi - lo) + lo
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1)


@pytest.mark.parametrize("variant,G,seed", [(0, 3, 1), (0, 8, 2), (1, 5, 3), (0, 40, 4)])
def test_rpn_restatement_equals_oracle_on_lattice_snapped_random_cases(variant, G, seed):
    """the inputs of test_rpn_targets_host_perm_parity, snapped: real anchor grids (many anchors collapse onto one lattice box, so
    ties are everywhere) and random gts.  Ties between different (inter, union) pairs of EQUAL ratio can occur here, which fp32
    also reports as equal in variant 1 only; so the guard is not asked, the two implementations are."""
    rng = np.random.RandomState(seed)
    if variant == 0:
        anchor = orc.anchor_grid(600, 1000)
    else:
        anchor = orc.tv_anchor_grid(320, 480, [(80, 120), (40, 60), (20, 30), (10, 15), (5, 8)], normalise=True)
    a = np.rint(np.asarray(anchor, np.float64) * tr.LAT).astype(np.int64)
    a = a[(a[:, 2] > a[:, 0]) & (a[:, 3] > a[:, 1])]
    c = tr.RpnCase("snapped", variant, a, _snap(_rand_gt(rng, G)), None)
    r = tr.rpn_match(c)
    assert r.n_neg > 256                                               # sampling happens
    _rpn_vs_oracle(c, [tr.rpn_perms(c, seed), _philox_rpn_perms(c, 7, seed)])


@pytest.mark.parametrize("variant,P", [(0, 2000), (0, 300), (1, 1000)])
def test_head_restatement_equals_oracle_on_lattice_snapped_random_cases(variant, P):
    rng = np.random.RandomState(P + variant)
    G = 5
    gt = _rand_gt(rng, G)
    lab = rng.randint(0, 20, G).astype(np.int64)
    rois = _rand_boxes(rng, P, 0.05, 0.5)
    rois[:40] = np.clip(gt[rng.randint(0, G, 40)] + rng.randn(40, 4) * 0.03, 0, 1)
    c = tr.HeadCase("snapped", variant, _snap(rois), _snap(gt), lab, None, n_rois=P - 13)
    r = tr.head_match(c)
    assert r.npc > 5 and r.nnc > c.total
    _head_vs_oracle(c, [tr.head_perms(c, "random"), _philox_head_perms(c, 3, 1)])


def test_the_guard_rejects_what_fp32_could_decide_differently():
    """the guard is not vacuous: (a) a row maximum 1000000/1001000 with 999000/1000000 one part in a million below it; (b) an argmax tie
    between DIFFERENT (inter, union) pairs of equal ratio, (1, 2) and (2, 4); (c) 0/0 in variant 1.  An exact 1/2 under eps is no
    exact hit but IS decidable: eps moves it clear of the threshold."""
    big = [0, 0, 1000, 1000]
    with pytest.raises(AssertionError, match="too close"):
        tr.check_decidable(tr.HeadCase("close", 1, [big], [[0, 0, 1001, 1000], [0, 0, 1000, 999]], [1, 2], None))
    with pytest.raises(AssertionError, match="shared by different"):
        tr.check_decidable(_equal_ratio_case())
    tr.check_decidable(tr.HeadCase("half-with-eps", 0, [[0, 0, 10, 20]], [[0, 0, 10, 10]], [1], None))
    with pytest.raises(AssertionError, match="0/0"):
        tr.check_decidable(tr.RpnCase("zero-over-zero", 1, [[3, 3, 3, 5], [0, 0, 4, 4]], [[8, 8, 8, 9], [0, 0, 4, 4]], None))


def _equal_ratio_case():
    """one RoI with IoU (1, 2) to the first gt and (2, 4) to the second: equal rationals from different integer pairs"""
    return tr.HeadCase("pairs", 1, [[0, 0, 2, 1]], [[0, 0, 1, 1], [0, 0, 2, 2]], [1, 2], None)
