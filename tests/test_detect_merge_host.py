"""CPU-only checks of the merge of detection sets (csrc/detect_merge.hip, include/frcnn_hip.h): the numpy restatement of the contract
(tests/detect_merge_ref.py) against hand-computed answers on dyadic data and against the oracle's NMS, its literal voting sums against
the naive float64 mean on exact data, and the C ABI's refusals and workspace sizes, which need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import detect_merge_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _set(boxes, labels, scores, count=None):
    b = np.array(boxes, F).reshape(-1, 4)
    return b, np.array(labels, np.int32), np.array(scores, F), len(b) if count is None else count


# ------------------------------------------------------------------------------------------------------------ 1. known answers
def test_ties_across_sets_keep_the_earlier_set_then_the_lower_row():
    a = _set([[0, 0, .25, .25], [.5, 0, .75, .25]], [0, 0], [.5, .5])
    b = _set([[0, .5, .25, .75], [0, 0, .25, .25]], [0, 0], [.5, .5])          # row 1 duplicates set 0's row 0
    r = ref.merge([a, b], [0, 0], 2)
    assert r["count"] == 3 and r["status"] == 0 and r["suppressed"] == 1
    assert r["boxes"].tolist() == [[0, 0, .25, .25], [.5, 0, .75, .25], [0, .5, .25, .75]]          # set 0 rows 0, 1, then set 1 row 0
    r = ref.merge([b, a], [0, 0], 2)                                            # the other way round: the duplicate of the EARLIER set survives
    assert r["boxes"].tolist() == [[0, .5, .25, .75], [0, 0, .25, .25], [.5, 0, .75, .25]]


def test_iou_exactly_at_the_threshold_is_kept_under_nms_and_votes():
    """A = [0, 0, .5, .5], B = [0, .125, .75, .875]: inter 3/16, union 5/8, IoU = fp32(0.3) exactly.  `> 0.3` is false, `>= 0.3` is true.
    Scores .75 and .25 sum to 1, so both voted boxes are .75 A + .25 B exactly."""
    s = _set([[0, 0, .5, .5], [0, .125, .75, .875]], [0, 0], [.75, .25])
    r = ref.merge([s], [0], 2, nms_thr=0.3)
    assert r["count"] == 2 and ref.same_bits(r["boxes"], s[0])
    assert ref.merge([s], [0], 2, nms_thr=0.2999)["count"] == 1
    r = ref.merge([s], [0], 2, nms_thr=0.3, vote_thr=0.3)
    want = np.array([[0, .03125, .5625, .59375]] * 2, F)
    assert r["voters"] == [2, 2] and ref.same_bits(r["boxes"], want) and ref.same_bits(r["unvoted"], s[0])
    assert ref.same_bits(r["scores"], s[2])
    r = ref.merge([s], [0], 2, nms_thr=0.3, vote_thr=0.3001)
    assert r["voters"] == [1, 1] and ref.same_bits(r["boxes"], s[0])


def test_flip_mirrors_the_box_back():
    s = _set([[.125, .125, .5, .625]], [1], [.5])
    assert ref.merge([s], [1], 3)["boxes"].tolist() == [[.5, .125, .875, .625]]
    assert ref.merge([s], [2], 3)["boxes"].tolist() == [[.125, .375, .5, .875]]
    assert ref.merge([s], [3], 3)["boxes"].tolist() == [[.5, .375, .875, .875]]
    assert ref.merge([s], [0], 3)["labels"].tolist() == [1] and ref.merge([s], [0], 3)["class_counts"].tolist() == [0, 1]
    # a mirrored copy of the same object meets the plain one: the later set is suppressed
    m = _set([[.5, .125, .875, .625]], [1], [.5])
    r = ref.merge([s, m], [0, 1], 3)
    assert r["count"] == 1 and r["suppressed"] == 1 and ref.same_bits(r["boxes"], s[0])


def test_self_only_voters_keep_their_bits():
    s = _set([[0, 0, .25, .25], [.5, .5, .75, .75], [np.nan, 0, .5, .5], [.25, .25, .25, .5], [-0.0, .75, .125, 1]], [0] * 5, [.9, .8, .7, .6, .5])
    r = ref.merge([s], [0], 2, vote_thr=0.5)
    assert r["count"] == 5 and r["voters"] == [1] * 5 and ref.same_bits(r["boxes"], s[0])          # NaN, zero-area and -0 rows included


def test_limits_and_status_bits():
    s = _set([[0, 0, .25, .25], [.5, .5, .75, .75]], [0, 5], [.5, .5])
    assert ref.merge([s], [0], 2)["status"] == ref.LABEL_RANGE
    assert ref.merge([(s[0], s[1], s[2], 3)], [0], 7)["status"] == ref.COUNT_CLIPPED
    r = ref.merge([(s[0], s[1], s[2], -1)], [0], 7)
    assert r["status"] == ref.UPSTREAM_ABORT and r["count"] == -1
    r = ref.merge([s], [0], 7, out_capacity=1)
    assert r["status"] == ref.OUTPUT_OVERFLOW and r["count"] == -1 and r["total"] == 2
    z = _set([[0, 0, .25, .25]] * 3, [0] * 3, [0.0, -1.0, np.nan])
    assert ref.merge([z], [0], 2)["count"] == 0                                 # strict `>`: 0, negative and NaN scores drop out


# ------------------------------------------------------------------------------------------------------------ 2. the oracle's NMS
def oracle_nms_of_concatenation(sets, C):
    """oracle.model_ref.ref_suppress on the concatenated live rows: row i of the concatenation is a candidate of class label + 1 only."""
    from oracle import model_ref
    b = np.concatenate([s[0][:s[3]] for s in sets])
    l = np.concatenate([s[1][:s[3]] for s in sets])
    sc = np.concatenate([s[2][:s[3]] for s in sets])
    R = len(l)
    raw = np.zeros((R, C, 4), F)
    prob = np.zeros((R, C), F)
    raw[np.arange(R), l + 1] = b
    prob[np.arange(R), l + 1] = sc
    return model_ref.ref_suppress(raw.reshape(R, C * 4), prob, C, 0.0)


@pytest.mark.parametrize("K,C,seed", [(2, 3, 1), (3, 21, 2)])
def test_nms_mode_equals_the_oracle_on_the_concatenation(K, C, seed):
    rng = np.random.RandomState(seed)
    sets = ref.random_sets(rng, K, C, [60 + 7 * k for k in range(K)], [50 + 5 * k for k in range(K)])
    r = ref.merge(sets, [0] * K, C, min_score=0.0, nms_thr=0.3)
    ob, ol, os_ = oracle_nms_of_concatenation(sets, C)
    assert r["count"] == len(ol) > 0 and r["suppressed"] > 0
    assert np.array_equal(r["labels"], ol) and ref.same_bits(r["scores"], os_) and ref.same_bits(r["boxes"], ob)


# ------------------------------------------------------------------------------------------------------------ 3. literal = naive on exact data
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 129])
def test_literal_and_naive_voting_agree_bit_for_bit_on_dyadic_data(m):
    rng = np.random.RandomState(m)
    sets = ref.dyadic_cluster(rng, m)
    a = ref.merge(sets, [0], 2, nms_thr=0.3, vote_thr=0.5)
    b = ref.merge(sets, [0], 2, nms_thr=0.3, vote_thr=0.5, naive=True)
    assert a["count"] == b["count"] > 0 and ref.same_bits(a["boxes"], b["boxes"])
    if m > 1:
        assert max(a["voters"]) == m and not ref.same_bits(a["boxes"], a["unvoted"])


# ------------------------------------------------------------------------------------------------------------ 4. the C ABI, no device
@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def test_workspace_bytes_of_the_merge(L):
    assert L.OP_DETECT_MERGE == 16 and L.lib.frcnn_abi_version() == 7
    for cap, C_ in [(12000, 21), (180000, 91), (1, 2), (0, 2), (100, 256)]:
        n = (C_ - 1) * max(1, min(cap, 2048))
        assert L.workspace_bytes(16, cap, C_) >= n * 20 + (C_ - 1) * 8
        assert L.workspace_bytes(16, cap, C_) <= n * 20 + (C_ - 1) * 8 + 5 * 256
    assert L.workspace_bytes(16, 100, 1) == 0 and L.workspace_bytes(16, 100, 257) == 0 and L.workspace_bytes(16, -1, 21) == 0


def test_c_abi_refusals_without_a_device(L):
    """Every refusal comes before the first launch, so made-up device addresses are never dereferenced."""
    f = L.lib.frcnn_detect_merge
    K, C_, cap = 2, 21, 100
    nb = L.workspace_bytes(16, cap, C_)
    dev = 0x10000                                                               # "device" addresses: 16-byte aligned, never read

    def call(K=K, C_=C_, cap=cap, caps=(50, 50), out_boxes=dev, boxes0=dev, nb=nb, ws=dev, rows=True):
        vp = C.c_void_p * 8
        row = lambda first: vp(*([first] + [dev] * 7)) if rows else None      # noqa: E731
        return f(K, row(boxes0), row(dev), row(dev), row(dev), (C.c_int64 * 8)(*(list(caps) + [1] * 6)), (C.c_uint32 * 8)(), C_, 0.0, 0.3, -1.0,
                 C.c_void_p(out_boxes), C.c_void_p(dev), C.c_void_p(dev), C.c_void_p(dev), None, None, cap, C.c_void_p(ws), nb, None)
    err = lambda: L.lib.frcnn_last_error()                                      # noqa: E731
    assert call(K=0) == -1 and b"K = 0" in err() and call(K=9) == -1              # FRCNN_ERR_INVALID_ARG
    assert call(out_boxes=None) == -1 and b"NULL" in err()
    assert call(boxes0=None) == -1 and b"NULL" in err() and call(rows=False) == -1 and call(ws=None) == -1
    assert call(caps=(50, -1)) == -1 and b"negative" in err() and call(cap=-1) == -1 and b"negative" in err()
    assert call(out_boxes=dev + 4) == -1 and b"aligned" in err() and call(boxes0=dev + 8) == -1
    assert call(C_=1) == -2 and call(C_=257) == -2 and b"C = 257" in err()       # FRCNN_ERR_UNSUPPORTED
    assert call(caps=(50, (1 << 28) + 1)) == -2
    assert call(nb=nb - 1) == -3 and b"workspace" in err()                        # FRCNN_ERR_WORKSPACE
