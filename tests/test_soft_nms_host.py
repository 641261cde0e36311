"""CPU-only checks of Soft-NMS as the merge's suppression step (csrc/detect_soft.hip, frcnn_detect_merge_soft in include/frcnn_hip.h):
the two numpy restatements of the contract (tests/soft_nms_ref.py) against each other, its hard mode against the restatement of the
greedy merge, hand-computed answers on dyadic data, the C ABI's refusals, which need no device, and the condition on the inputs of the
GPU tests of gaussian mode: every one has a margin above 1e-4."""
import ctypes as C
import os

import numpy as np
import pytest

import detect_merge_ref as mref
import soft_nms_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _set(boxes, scores):
    b = np.array(boxes, F).reshape(-1, 4)
    return b, np.zeros(len(b), np.int32), np.array(scores, F), len(b)


def _same(a, b, keys=("boxes", "labels", "scores", "class_counts")):
    return a["count"] == b["count"] and a["status"] == b["status"] and all(ref.same_bits(a[k], b[k]) for k in keys)


def _data(kind, seed):
    rng = np.random.RandomState(seed)
    if kind == "random":
        sets = ref.random_sets(rng, 2, 4, [80, 90], [70, 85], spread=0.15)
        return [(ref.flip(b, f), l, s, n) for (b, l, s, n), f in zip(sets, [0, 1])], [0, 1], 4
    if kind == "dyadic":
        return ref.random_sets(rng, 2, 3, [60, 60], [55, 50], dyadic=True, spread=0.15), [0, 0], 3
    return ref.dyadic_cluster(rng, 40), [0], 2


# ------------------------------------------------------------------------------------------------------------ 1. the two restatements
@pytest.mark.parametrize("vote", [None, 0.8], ids=["novote", "vote"])
@pytest.mark.parametrize("method", [ref.HARD, ref.LINEAR], ids=["hard", "linear"])
@pytest.mark.parametrize("kind,seed", [("random", 1), ("random", 2), ("dyadic", 3), ("cluster", 4)])
def test_the_two_restatements_agree_bit_for_bit(kind, seed, method, vote):
    sets, flags, C_ = _data(kind, seed)
    a = ref.soft_merge(sets, flags, C_, method, nms_thr=0.3, vote_thr=vote)
    b = ref.soft_merge(sets, flags, C_, method, nms_thr=0.3, vote_thr=vote, literal=True)
    assert a["count"] > 0 and _same(a, b)
    if method == ref.LINEAR:
        assert np.array_equal(a["decays"], b["decays"]) and a["decays"].max() >= 2          # the data do decay, more than once


@pytest.mark.parametrize("vote", [None, 0.8], ids=["novote", "vote"])
@pytest.mark.parametrize("kind,seed", [("random", 1), ("dyadic", 3), ("cluster", 4)])
def test_hard_mode_is_the_greedy_merge_bit_for_bit(kind, seed, vote):
    sets, flags, C_ = _data(kind, seed)
    a = ref.soft_merge(sets, flags, C_, ref.HARD, nms_thr=0.3, vote_thr=vote)
    g = mref.merge(sets, flags, C_, nms_thr=0.3, vote_thr=vote)
    assert g["suppressed"] > 0 and _same(a, g, keys=("boxes", "labels", "scores", "class_counts", "unvoted"))


@pytest.mark.parametrize("method", [ref.HARD, ref.LINEAR, ref.GAUSSIAN], ids=["hard", "linear", "gaussian"])
def test_emitted_scores_do_not_increase_inside_a_class(method):
    sets, flags, C_ = _data("random", 5)
    r = ref.soft_merge(sets, flags, C_, method)
    assert r["count"] > 20
    for c in range(C_ - 1):
        s = r["scores"][r["labels"] == c].astype(np.float64)
        assert len(s) > 1 and (np.diff(s) <= 0).all()


# ------------------------------------------------------------------------------------------------------------ 2. known answers
A_, B_, C_BOX = [0, 0, .5, .5], [0, 0, .5, .25], [.75, .75, 1, 1]             # IoU(A, B) = (1/8) / (1/4) = 0.5 exactly; C touches neither


def test_linear_mode_known_answer_on_dyadic_boxes():
    """A (.75) is picked; B decays to s_B * (1 - 0.5); C is untouched.  All scores are exact binary fractions."""
    r = ref.soft_merge([_set([A_, B_, C_BOX], [.75, .625, .25])], [0], 2, ref.LINEAR, nms_thr=0.3)
    assert r["scores"].tolist() == [.75, .3125, .25] and r["boxes"].tolist() == [A_, B_, C_BOX] and r["decays"].tolist() == [0, 1, 0]
    # the decay reorders: B falls behind C -- one sort up front would not do
    r = ref.soft_merge([_set([A_, B_, C_BOX], [.75, .375, .25])], [0], 2, ref.LINEAR, nms_thr=0.3)
    assert r["scores"].tolist() == [.75, .25, .1875] and r["boxes"].tolist() == [A_, C_BOX, B_] and r["decays"].tolist() == [0, 0, 1]
    # B decays onto C's score exactly: the lower sorted position first
    r = ref.soft_merge([_set([A_, B_, C_BOX], [.75, .5, .25])], [0], 2, ref.LINEAR, nms_thr=0.3)
    assert r["scores"].tolist() == [.75, .25, .25] and r["boxes"].tolist() == [A_, B_, C_BOX] and r["margin"] == 0.0
    r = ref.soft_merge([_set([A_, C_BOX, B_], [.75, .25, .5])], [0], 2, ref.LINEAR, nms_thr=0.3)          # rows swapped: B still sorts before C
    assert r["boxes"].tolist() == [A_, B_, C_BOX]
    # IoU exactly at the threshold decays nothing; hard mode at 0.5 keeps B, just below it drops B
    assert ref.soft_merge([_set([A_, B_, C_BOX], [.75, .5, .25])], [0], 2, ref.LINEAR, nms_thr=0.5)["scores"].tolist() == [.75, .5, .25]
    assert ref.soft_merge([_set([A_, B_, C_BOX], [.75, .5, .25])], [0], 2, ref.HARD, nms_thr=0.5)["count"] == 3
    assert ref.soft_merge([_set([A_, B_, C_BOX], [.75, .5, .25])], [0], 2, ref.HARD, nms_thr=0.4999)["count"] == 2


def test_the_floor_keeps_an_equal_score_and_drops_one_ulp_below():
    s = [_set([A_, B_, C_BOX], [.75, .5, .125])]
    assert ref.soft_merge(s, [0], 2, ref.LINEAR, floor=0.25)["scores"].tolist() == [.75, .25, .125]          # C was never decayed: no floor for it
    assert ref.soft_merge(s, [0], 2, ref.LINEAR, floor=float(np.nextafter(F(0.25), F(1))))["scores"].tolist() == [.75, .125]


def test_gaussian_mode_known_answer():
    r = ref.soft_merge([_set([A_, B_, C_BOX], [.75, .5, .25])], [0], 2, ref.GAUSSIAN, sigma=0.5)
    want = F(F(.5) * F(np.exp(-0.25 / 0.5)))
    assert r["boxes"].tolist() == [A_, B_, C_BOX] and r["scores"].tolist() == [.75, float(want), .25] and r["decays"].tolist() == [0, 1, 0]


# ------------------------------------------------------------------------------------------------------------ 3. the GPU tests' inputs
def test_every_gaussian_input_of_the_gpu_tests_has_a_margin_above_1e_4():
    cases = ref.gaussian_cases()
    assert len(cases) >= 4
    for name, sets, flags, C_, kw in cases:
        r = ref.soft_merge(sets, flags, C_, ref.GAUSSIAN, **kw)
        per_class = np.bincount(np.concatenate([l[:n] for _, l, _, n in sets]), minlength=C_ - 1)
        assert per_class.max() <= 64, (name, per_class)
        assert r["margin"] > 1e-4, (name, r["margin"])
        assert r["count"] > 0 and r["status"] == 0 and r["decays"].max() >= 3, name            # and is no degenerate case


# ------------------------------------------------------------------------------------------------------------ 4. the C ABI, no device
@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def test_constants_and_the_value_object(L):
    from faster_rcnn_pytorch_amd import ops
    assert (L.SOFT_NMS_HARD, L.SOFT_NMS_LINEAR, L.SOFT_NMS_GAUSSIAN) == (ref.HARD, ref.LINEAR, ref.GAUSSIAN) == (0, 1, 2)
    s = ops.SoftNMS()
    assert (s.method, s.sigma, s.score_floor, s.code) == ("linear", 0.5, 1e-3, 1)
    assert ops.SoftNMS("gaussian", 0.3).code == 2 and ops.SoftNMS("hard", sigma=-1).code == 0          # sigma is read in gaussian mode only
    for bad in (dict(method="exp"), dict(method="gaussian", sigma=0.0), dict(method="gaussian", sigma=float("nan")), dict(score_floor=float("nan"))):
        with pytest.raises(ValueError):
            ops.SoftNMS(**bad)


def test_c_abi_refusals_without_a_device(L):
    """Every refusal comes before the first launch, so made-up device addresses are never dereferenced."""
    f = L.lib.frcnn_detect_merge_soft
    K, C_, cap = 2, 21, 100
    nb = L.workspace_bytes(16, cap, C_)
    dev = 0x10000                                                               # "device" addresses: 16-byte aligned, never read

    def call(K=K, C_=C_, cap=cap, caps=(50, 50), out_boxes=dev, boxes0=dev, nb=nb, ws=dev, rows=True, method=1, sigma=0.5, floor=1e-3):
        vp = C.c_void_p * 8
        row = lambda first: vp(*([first] + [dev] * 7)) if rows else None      # noqa: E731
        return f(K, row(boxes0), row(dev), row(dev), row(dev), (C.c_int64 * 8)(*(list(caps) + [1] * 6)), (C.c_uint32 * 8)(), C_, 0.0, 0.3, -1.0,
                 method, sigma, floor, C.c_void_p(out_boxes), C.c_void_p(dev), C.c_void_p(dev), C.c_void_p(dev), None, None, cap, C.c_void_p(ws), nb,
                 None)
    err = lambda: L.lib.frcnn_last_error()                                      # noqa: E731
    assert call(method=3) == -1 and b"method = 3" in err() and call(method=-1) == -1              # FRCNN_ERR_INVALID_ARG
    assert call(method=2, sigma=0.0) == -1 and b"sigma" in err() and call(method=2, sigma=-1.0) == -1
    assert call(method=2, sigma=float("nan")) == -1 and b"sigma" in err()
    assert call(floor=float("nan")) == -1 and b"score_floor" in err()
    # frcnn_detect_merge's own refusals
    assert call(K=0) == -1 and b"K = 0" in err() and call(K=9) == -1
    assert call(out_boxes=None) == -1 and b"NULL" in err()
    assert call(boxes0=None) == -1 and b"NULL" in err() and call(rows=False) == -1 and call(ws=None) == -1
    assert call(caps=(50, -1)) == -1 and b"negative" in err() and call(cap=-1) == -1 and b"negative" in err()
    assert call(out_boxes=dev + 4) == -1 and b"aligned" in err() and call(boxes0=dev + 8) == -1
    assert call(C_=1) == -2 and call(C_=257) == -2 and b"C = 257" in err()       # FRCNN_ERR_UNSUPPORTED
    assert call(caps=(50, (1 << 28) + 1)) == -2
    assert call(nb=nb - 1) == -3 and b"workspace" in err()                        # FRCNN_ERR_WORKSPACE
