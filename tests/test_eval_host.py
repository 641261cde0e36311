"""CPU-only checks of the detection evaluator (faster_rcnn_pytorch_amd/evaluation.py, csrc/eval.hip): the restatement of the VOC AP
protocol the GPU tests compare against (tests/eval_ref.py) equals the reference's own evaluator on the golden set
(tests/golden/voc_eval.npz, written by tests/golden/make_golden_voc_eval.py from evaluation/voc_eval.py), its per-frame form equals
its sequential form flag for flag, and the two new entry points are declared, exported, bound and refuse bad arguments without a
device."""
import os
import re
import subprocess

import numpy as np
import pytest

import eval_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def test_golden_set_contains_every_adverse_kind(golden):
    z = golden("voc_eval")
    kinds = dict(zip([str(k) for k in z["adverse_kinds"]], z["adverse_counts"].tolist()))
    for k in ("tied_scores_within_image", "tied_scores_across_images", "identical_gt_boxes", "best_match_difficult", "second_on_used_gt",
              "ov_just_below_threshold", "ov_just_above_threshold", "ov_equal_threshold", "class_dets_without_npos", "class_gt_without_dets",
              "image_without_gt", "image_without_det"):
        assert kinds[k] >= 1, k
    assert z["thresholds"].tolist() == [0.3, 0.5, 0.75]
    assert np.isnan(z["ap"][:, z["npos"] == 0]).all() and not np.isnan(z["ap"][:, z["npos"] > 0]).any()


def test_sequential_restatement_equals_the_reference(golden):
    """The same float64 operations in the same order: per-class AP within 1e-15 of cal_mAP's (it is equal), NaN in the same places."""
    z = golden("voc_eval")
    frames = eval_ref.frames_from_golden(z)
    nc, thr = int(z["num_classes"]), z["thresholds"].tolist()
    rec, npos = eval_ref.sequential(frames, nc, thr)
    assert np.array_equal(npos, z["npos"])
    ap, mean = eval_ref.average_precision(rec, npos, len(thr))
    assert np.array_equal(np.isnan(ap), np.isnan(z["ap"]))
    known = ~np.isnan(ap)
    assert np.abs(ap[known] - z["ap"][known]).max() <= 1e-15
    assert np.abs(mean - z["map"]).max() <= 1e-15
    assert len(rec["label"]) == len(z["det_labels"])


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_parallel_form_equals_sequential_flag_for_flag(seed, golden):
    """Per-image independence: TP iff first, in (score desc, position asc), of the frame's detections sharing the match and reaching t."""
    if seed == 0:
        z = golden("voc_eval")
        frames, nc = eval_ref.frames_from_golden(z), int(z["num_classes"])
    else:
        frames, nc = eval_ref.make_set(seed, n_images=30, num_classes=6, quantise=0.1 if seed % 2 else 0.0, difficult=0.25), 6
    thr = (0.3, 0.5, 0.75)
    a, na = eval_ref.sequential(frames, nc, thr)
    b, nb = eval_ref.parallel(frames, nc, thr)
    assert np.array_equal(na, nb)
    for k in ("label", "score", "image_id", "position", "flags"):
        assert np.array_equal(a[k], b[k]), k
    assert set(np.unique((a["flags"] >> 2) & 3)) <= {eval_ref.TP, eval_ref.FP, eval_ref.IGNORED}
    # the order is the contract: (label asc, score desc, image_id asc, position asc)
    key = list(zip(a["label"].tolist(), (-a["score"].astype(np.float64)).tolist(), a["image_id"].tolist(), a["position"].tolist()))
    assert key == sorted(key)


def test_vectorised_overlaps_equal_the_literal_loop(golden):
    """tests/eval_ref.py's numpy form of the match (used for the 6000-detection frames of the GPU tests) against its literal loop."""
    sets = [eval_ref.frames_from_golden(golden("voc_eval")), eval_ref.make_set(7, n_images=20), [eval_ref.make_big_frame(3, 400, 64, 4)]]
    for frames in sets:
        for f in frames:
            assert eval_ref._frame_matches(f) == eval_ref._frame_matches_np(f)
    f = eval_ref.make_big_frame(3, 400, 64, 4)
    a, _ = eval_ref.parallel([f], 4, (0.3, 0.5))
    b, _ = eval_ref.parallel([f], 4, (0.3, 0.5), fast=True)
    c, _ = eval_ref.sequential([f], 4, (0.3, 0.5))
    assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["flags"], c["flags"])
    assert ((a["flags"] & 3) == eval_ref.TP).sum() > 10 and ((a["flags"] & 3) == eval_ref.IGNORED).sum() > 10


def test_symbols_declared_exported_and_bound(L):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    for sym in ("frcnn_eval_update", "frcnn_eval_average_precision"):
        assert re.search(r"\b%s\s*\(" % sym, txt), sym
        assert re.search(r" T %s\b" % sym, out), sym
        assert sym in L.SIGNATURES
    assert "FRCNN_OP_EVAL = 12" in txt and L.OP_EVAL == 12
    assert (L.EVAL_TP, L.EVAL_FP, L.EVAL_IGNORED) == (eval_ref.TP, eval_ref.FP, eval_ref.IGNORED)


def test_abi_version_is_still_7(L):
    assert L.lib.frcnn_abi_version() == L.ABI_VERSION == 7


P = 0x1000          # a non-NULL pointer that is never dereferenced: every refusal below happens before a launch


def _update(L, T=1, C=21, D=300, G=64, cap=1000, null=()):
    a = {k: P for k in ("boxes", "labels", "scores", "count", "gtb", "gtl", "gtd", "ngt", "frame", "thr", "npos", "rs", "rl", "ri", "rp", "rf",
                        "cursor", "err", "ws")}
    for k in null:
        a[k] = None
    return L.lib.frcnn_eval_update(a["boxes"], a["labels"], a["scores"], a["count"], D, a["gtb"], a["gtl"], a["gtd"], a["ngt"], G, a["frame"],
                                   a["thr"], T, C, a["npos"], a["rs"], a["rl"], a["ri"], a["rp"], a["rf"], cap, a["cursor"], a["err"], a["ws"],
                                   1 << 30, None)


def _ap(L, T=1, C=21, cap=1000, null=()):
    a = {k: P for k in ("lab", "fl", "n", "npos", "ap", "tp", "fp", "ws")}
    for k in null:
        a[k] = None
    return L.lib.frcnn_eval_average_precision(a["lab"], a["fl"], a["n"], cap, a["npos"], T, C, a["ap"], a["tp"], a["fp"], a["ws"], 1 << 30, None)


def test_update_refuses_null_outputs(L):
    for k in ("npos", "rs", "rl", "ri", "rp", "rf", "cursor", "err", "ws", "boxes", "thr"):
        assert _update(L, null=(k,)) == -1 and b"eval_update" in L.lib.frcnn_last_error(), k


def test_average_precision_refuses_null_outputs(L):
    for k in ("ap", "tp", "fp", "ws", "lab", "n"):
        assert _ap(L, null=(k,)) == -1 and b"eval_average_precision" in L.lib.frcnn_last_error(), k


def test_threshold_count_0_and_17_refused(L):
    assert _update(L, T=0) == -2 and _update(L, T=17) == -2
    assert _ap(L, T=0) == -2 and _ap(L, T=17) == -2


def test_gt_capacity_1025_refused(L):
    assert _update(L, G=1025) == -2 and b"eval_update" in L.lib.frcnn_last_error()
    assert _update(L, G=0) == -2


def test_class_count_1_and_257_refused(L):
    assert _update(L, C=1) == -2 and _update(L, C=257) == -2
    assert _ap(L, C=1) == -2 and _ap(L, C=257) == -2


def test_detection_capacity_beyond_detect_postprocess_refused(L):
    assert _update(L, C=21, D=20 * 2048 + 1) == -2              # (C-1) * P, P <= 2048
    assert _update(L, C=21, D=0) == -2


def test_workspace_bytes_zero_outside_the_limits(L):
    assert L.workspace_bytes(L.OP_EVAL, 6000, 1024) >= 16 * 1024 * 8 + 6000 * 8
    assert L.workspace_bytes(L.OP_EVAL, 255 * 2048, 1024) > 0
    assert L.workspace_bytes(L.OP_EVAL, 255 * 2048 + 1, 64) == 0
    assert L.workspace_bytes(L.OP_EVAL, 300, 1025) == 0
    assert L.workspace_bytes(L.OP_EVAL, 0, 64) == 0 and L.workspace_bytes(L.OP_EVAL, 300, 0) == 0


def test_small_workspace_refused(L):
    a = [P] * 4 + [300] + [P] * 4 + [64, P, P, 1, 21] + [P] * 6 + [1000, P, P, P, 16, None]
    assert L.lib.frcnn_eval_update(*a) == -3


def test_evaluator_refuses_bad_configuration_without_a_device(L):
    from faster_rcnn_pytorch_amd import evaluation
    with pytest.raises(ValueError):
        evaluation.DetectionEvaluator(21, iou_thresholds=())
    with pytest.raises(ValueError):
        evaluation.DetectionEvaluator(21, iou_thresholds=[0.5] * 17)
    with pytest.raises(ValueError):
        evaluation.DetectionEvaluator(257)
    with pytest.raises(ValueError):
        evaluation.DetectionEvaluator(21, gt_capacity=1025)
    with pytest.raises(ValueError):
        evaluation.GroundTruth(1025, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.DetectionEvaluator(21, device="cpu")


def test_tree_names_nothing_that_is_off_limits():
    """The new sources hold no scalar-store / scalar-atomic mnemonic, no XNACK or debugger use and do not name the graph-queue debug
    variable (the words are assembled here so that this file does not contain them either)."""
    words = ["s_" + w for w in ("store_dword", "buffer_store", "scratch_store", "atomic_", "buffer_atomic", "dcache_wb", "dcache_discard")]
    words += ["HSA_" + "XNACK", "xnack" + "+", "roc" + "gdb", "DEBUG_HIP_" + "FORCE_GRAPH_QUEUES"]
    for rel in ("faster_rcnn_pytorch_amd/csrc/eval.hip", "faster_rcnn_pytorch_amd/evaluation.py", "faster_rcnn_pytorch_amd/inference.py",
                "tests/eval_ref.py", "tests/test_gpu_eval.py", "tools/infer_bench.py"):
        txt = open(os.path.join(ROOT, rel)).read().lower()
        for w in words:
            assert w.lower() not in txt, (rel, w)
