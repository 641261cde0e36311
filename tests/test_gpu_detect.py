"""The fused detection post-process (csrc/detect.hip, ops.detect_postprocess), FRCNN.detect in both mirrors and DetectGraph,
against the oracle's restatement of FRCNN.predict's post-processing (oracle/model_ref.py: ref_predict_post / ref_suppress) and
against predict itself.  The kernel's own softmax is handed to the oracle (prob=) so that the logic under test -- decode, clamp,
thresholding, per-class NMS, class-major order -- is compared bit for bit."""

import numpy as np
import pytest
import torch

from oracle import model_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.as_tensor(a, dtype=dtype).to(DEV)


def _same_bits(a, b):
    """Equal shapes, NaN in the same places, every other value bit-identical (-0 and +0 differ)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(np.uint32), np.where(nb, 0, b).view(np.uint32))


def _inputs(P, C, seed, n=None):
    rng = np.random.RandomState(seed)
    hc = (rng.randn(P, C) * 0.8).astype(np.float32)
    hr = (rng.randn(P, 4 * C) * 0.5).astype(np.float32)
    c = rng.rand(P, 2) * 0.8 + 0.1
    wh = rng.rand(P, 2) * 0.5 + 0.05
    rois = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)
    if n is not None and n < P:                       # the head ran on padded rows: garbage and NaN there
        hc[n:] = np.nan
        hc[n::2] = 1e30
        hr[n:] = np.float32(3e38)
        rois[n:] = np.nan
    return hc, hr, rois


def _run(hc, hr, rois, n, thr, nms=0.3, thr_dev=None):
    from faster_rcnn_pytorch_amd import ops
    return ops.detect_postprocess(_t(hc), _t(hr), _t(rois), _t([n], torch.int32), thr, nms, threshold_dev=thr_dev, want_prob=True)


def _check_vs_oracle(hc, hr, rois, n, thr, want_nonempty=True):
    C_ = hc.shape[1]
    det = _run(hc, hr, rois, n, thr)
    prob = det.prob.cpu().numpy()
    b, l, s = det.to_host()
    count, cc = int(det.count.item()), det.class_counts.cpu().numpy()
    if n == 0:
        assert count == 0 and (cc == 0).all() and b.shape == (0, 4)
        return det
    rb, rl, rs, _, _ = model_ref.ref_predict_post(hc[:n], hr[:n], rois[:n], C_, thr, prob=prob[:n])
    assert count == len(rl) and np.array_equal(cc, np.bincount(rl, minlength=C_ - 1))
    assert np.array_equal(l.numpy(), rl)                                           # class-major, (l - 1), score order
    assert _same_bits(s.numpy(), rs) and _same_bits(b.numpy(), rb)
    if want_nonempty:
        assert len(rl) > 0
    # the kernel's softmax against torch's, on the device and on the CPU (live rows)
    live = np.isfinite(hc[:n]).all(1)
    dev_sm = torch.softmax(_t(hc[:n]), dim=-1).cpu().numpy()
    cpu_sm = torch.softmax(torch.from_numpy(hc[:n]), dim=-1).numpy()
    assert np.abs(prob[:n][live] - dev_sm[live]).max(initial=0) < 1e-6
    assert np.abs(prob[:n][live] - cpu_sm[live]).max(initial=0) < 1e-6
    assert np.array_equal(np.isnan(prob[:n]), np.isnan(dev_sm))
    return det


# ------------------------------------------------------------------------------------------------------------ 1. the op vs the oracle
@pytest.mark.parametrize("P,C,thr,seed", [(300, 21, 0.05, 1), (1000, 91, 0.02, 2), (7, 3, 0.05, 3)], ids=["vgg_300x21", "fpn_1000x91", "7x3"])
def test_detect_postprocess_matches_oracle(P, C, thr, seed):
    hc, hr, rois = _inputs(P, C, seed)
    det = _check_vs_oracle(hc, hr, rois, P, thr)
    assert det.boxes.shape == ((C - 1) * P, 4) and det.labels.dtype == torch.int32 and det.count.dtype == torch.int32


def test_detect_postprocess_ignores_padded_rows():
    hc, hr, rois = _inputs(300, 21, 4, n=173)
    _check_vs_oracle(hc, hr, rois, 173, 0.05)


def test_detect_postprocess_no_live_rows_and_a_threshold_that_keeps_nothing():
    hc, hr, rois = _inputs(300, 21, 5, n=0)
    _check_vs_oracle(hc, hr, rois, 0, 0.05)
    hc, hr, rois = _inputs(300, 21, 5)
    det = _check_vs_oracle(hc, hr, rois, 300, 0.999, want_nonempty=False)
    assert int(det.count.item()) == 0


@pytest.mark.parametrize("P,C", [(300, 21), (2048, 4)])
def test_detect_postprocess_every_pair_a_candidate(P, C):
    """threshold -1: all (C-1) P pairs are candidates (2048 per class at the largest P: the whole bitonic sort)."""
    hc, hr, rois = _inputs(P, C, 6)
    _check_vs_oracle(hc, hr, rois, P, -1.0)
    # nms_threshold above any IoU: nothing is suppressed, the full (C-1) P output capacity is used, in (score desc, row asc) order
    det = _run(hc, hr, rois, P, -1.0, nms=1.5)
    b, l, s = det.to_host()
    prob = det.prob.cpu().numpy()
    assert len(l) == (C - 1) * P
    for c in range(1, C):
        order = np.argsort(-prob[:, c], kind="stable")
        sel = l.numpy() == c - 1
        assert np.array_equal(s.numpy()[sel], prob[order, c])


# ------------------------------------------------------------------------------------------------------------ 2. known answers
def test_exact_score_ties_keep_ascending_rows():
    """Rows 4..7 duplicate rows 0..3 (logits, deltas and box): equal scores, the duplicates are suppressed (IoU 1) and the four
    disjoint boxes are kept in ascending row order."""
    P, C_ = 8, 3
    hc = np.tile(np.array([[0.0, 1.0, 0.5]], np.float32), (P, 1))
    hr = np.zeros((P, 4 * C_), np.float32)
    rois = np.array([[0.2 * i, 0.1, 0.2 * i + 0.125, 0.5] for i in range(4)] * 2, np.float32)
    det = _check_vs_oracle(hc, hr, rois, P, 0.05)
    b, l, s = det.to_host()
    assert l.tolist() == [0] * 4 + [1] * 4
    bx = b.numpy()
    assert np.array_equal(bx[:4], bx[4:]) and (np.diff(bx[:4, 0]) > 0).all()                      # rows 0, 1, 2, 3 in that order
    assert len(set(s.numpy()[:4].tolist())) == 1


def test_iou_exactly_at_the_threshold_is_not_suppressed():
    """A = [0, 0, .5, .5], B = [0, .125, .75, .875]: inter 3/16, union 5/8, IoU = fp32(0.3) exactly: `> 0.3` is false."""
    hc = np.array([[0.0, 2.0], [0.0, 1.0]], np.float32)
    hr = np.zeros((2, 8), np.float32)
    rois = np.array([[0, 0, 0.5, 0.5], [0, 0.125, 0.75, 0.875]], np.float32)
    det = _check_vs_oracle(hc, hr, rois, 2, 0.05)
    assert int(det.count.item()) == 2 and np.array_equal(det.to_host()[0].numpy(), rois)
    assert int(_run(hc, hr, rois, 2, 0.05, nms=0.2999).count.item()) == 1


def test_nan_logits_and_nan_deltas_follow_the_oracle():
    P, C_ = 64, 5
    hc, hr, rois = _inputs(P, C_, 7)
    hc[3, 2] = np.nan                         # a NaN logit: the whole row's softmax is NaN, no candidate
    hc[9, :] = np.nan
    hr[5, 4:8] = np.nan                       # class 1 box of row 5 is NaN: a candidate that suppresses nothing
    hr[11, 8 + 2] = np.nan
    hc[5, 1] = hc[11, 2] = 4.0                # make those rows candidates
    _check_vs_oracle(hc, hr, rois, P, 0.05)


def test_aborted_proposal_scan_gives_count_minus_one():
    from faster_rcnn_pytorch_amd import _lib
    hc, hr, rois = _inputs(300, 21, 8)
    det = _run(hc, hr, rois, -1, 0.05)
    assert int(det.count.item()) == -1
    with pytest.raises(_lib.FrcnnError):
        det.to_host()


def test_device_threshold_overrides_the_host_value():
    hc, hr, rois = _inputs(300, 21, 9)
    a = _run(hc, hr, rois, 300, 0.9, thr_dev=_t([0.05], torch.float32)).to_host()
    b = _run(hc, hr, rois, 300, 0.05).to_host()
    assert len(a[1]) > 0 and all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------ 5. C ABI refusals
def test_c_abi_refusals():
    from faster_rcnn_pytorch_amd import _lib
    from faster_rcnn_pytorch_amd.ops import _ptr, _stream
    f = _lib.lib.frcnn_detect_postprocess
    P, C_ = 300, 21
    hc, hr, ro = torch.zeros(P, C_, device=DEV), torch.zeros(P, 4 * C_, device=DEV), torch.zeros(P, 4, device=DEV)
    n = torch.full((1,), P, dtype=torch.int32, device=DEV)
    ob, ol, os_ = torch.empty((C_ - 1) * P, 4, device=DEV), torch.empty((C_ - 1) * P, dtype=torch.int32, device=DEV), torch.empty((C_ - 1) * P, device=DEV)
    cnt = torch.empty(1, dtype=torch.int32, device=DEV)
    nb = _lib.workspace_bytes(_lib.OP_DETECT, P, C_)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)

    def call(P_=P, C__=C_, out_boxes=ob, wsb=nb):
        return f(_ptr(hc), _ptr(hr), _ptr(ro), _ptr(n), P_, C__, 0.01, None, 0.3, _ptr(out_boxes), _ptr(ol), _ptr(os_), _ptr(cnt), None, None,
                 _ptr(ws), wsb, _stream())
    assert call(P_=2049) == -2 and call(C__=257) == -2                                            # FRCNN_ERR_UNSUPPORTED
    assert _lib.workspace_bytes(_lib.OP_DETECT, 2049, C_) == 0 and _lib.workspace_bytes(_lib.OP_DETECT, P, 257) == 0
    assert call(out_boxes=None) == -1 and b"NULL" in _lib.lib.frcnn_last_error()                  # FRCNN_ERR_INVALID_ARG
    assert call(wsb=nb - 1) == -3 and b"workspace" in _lib.lib.frcnn_last_error()                 # FRCNN_ERR_WORKSPACE
    assert call() == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == (C_ - 1) * P          # prob 1/21 > 0.01 everywhere; zero-area boxes: IoU 0/0 = NaN suppresses nothing


# ------------------------------------------------------------------------------------------------------------ 3. model level
@pytest.fixture(scope="module")
def vgg():
    from faster_rcnn_pytorch_amd.model import FRCNN
    torch.manual_seed(0)
    m = FRCNN(num_classes=21, sampling="host").to(DEV)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():                        # as tests/test_gpu_model.py: non-trivial RPN outputs, spread head logits and deltas
        m.rpn.cls_layer.weight.mul_(30)
        m.rpn.reg_layer.weight.mul_(10)
        m.fast_rcnn_head.cls_head.weight.copy_(torch.randn(m.fast_rcnn_head.cls_head.weight.shape, generator=g) * 0.8)
        m.fast_rcnn_head.reg_head.weight.copy_(torch.randn(m.fast_rcnn_head.reg_head.weight.shape, generator=g) * 0.5)
    return m.eval()


@pytest.fixture(scope="module")
def fpn():
    from faster_rcnn_pytorch_amd.new_model import FRCNN
    torch.manual_seed(0)
    m = FRCNN(num_classes=91, sampling="host").to(DEV)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        m.rpn.rpn_head.cls_layer.weight.mul_(30)
        m.rpn.rpn_head.reg_layer.weight.mul_(2)
        m.frcnn_head.cls_head.weight.copy_(torch.randn(m.frcnn_head.cls_head.weight.shape, generator=g) * 0.8)
        m.frcnn_head.reg_head.weight.copy_(torch.randn(m.frcnn_head.reg_head.weight.shape, generator=g) * 0.5)
    return m.eval()


def _frame(seed, H, W):
    return torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(seed))


def _head(m):
    return m.fast_rcnn_head if hasattr(m, "fast_rcnn_head") else m.frcnn_head


def _detect_vs_predict(m, x, thres, num_classes):
    head = _head(m)
    cap = {}
    h = head.register_forward_hook(lambda mod, i, o: cap.setdefault("outs", []).append((i[1].detach().clone(), o[0].detach().float().clone(),
                                                                                        o[1].detach().float().clone())))
    try:
        pb, pl, ps = m.predict(x.to(DEV), thres)
        det = m.detect(x.to(DEV), thres, want_prob=True)
        db, dl, ds = det.to_host()
    finally:
        h.remove()
    (p_rois, p_hc, p_hr), (d_rois, d_hc, d_hr) = cap["outs"]
    n = int(det.n_rois.item())
    assert n == p_rois.shape[0] and d_rois.shape[0] >= n and torch.equal(d_rois[:n], p_rois)
    prob = det.prob.cpu().numpy()
    # (a) detect with the head hooked: the oracle on detect's own head outputs and softmax, bit-exact
    rb, rl, rs, _, _ = model_ref.ref_predict_post(d_hc[:n].cpu().numpy(), d_hr[:n].cpu().numpy(), d_rois[:n].cpu().numpy(), num_classes, thres,
                                                  prob=prob[:n])
    assert len(rl) > 20 and len(np.unique(rl)) > 1, "degenerate test frame"
    assert np.array_equal(dl.numpy(), rl) and _same_bits(ds.numpy(), rs) and _same_bits(db.numpy(), rb)
    # (b) detect against predict.  The post-process is exact (a); what can differ is the head itself: detect runs it on all P rows,
    # predict on the first n, and the GEMM behind nn.Linear may pick another reduction order for another row count (seen with the
    # FPN mirror, n < P = 1000).  Same head rows: boxes bit-identical, scores within 1e-6.  Otherwise boxes within 1e-4.
    same_head = torch.equal(d_hc[:n], p_hc) and torch.equal(d_hr[:n], p_hr)
    if not same_head:
        assert (d_hc[:n] - p_hc).abs().max() <= 1e-5 * max(1.0, float(p_hc.abs().max()))
        assert (d_hr[:n] - p_hr).abs().max() <= 1e-5 * max(1.0, float(p_hr.abs().max()))
    p_prob = torch.softmax(p_hc, dim=-1).cpu().numpy()
    assert np.abs(prob[:n] - p_prob).max() < 1e-6
    diff = (p_prob[:, 1:] > thres) != (prob[:n, 1:] > thres)
    if diff.sum() == 0 and np.array_equal(dl.numpy(), pl.numpy()):
        if same_head:
            assert _same_bits(db.numpy(), pb.numpy())
        else:
            assert np.abs(db.numpy() - pb.numpy()).max(initial=0) < 1e-4          # the model tests' box tolerance (test_gpu_model.py)
        assert np.abs(ds.numpy() - ps.numpy()).max(initial=0) < 1e-6
    else:                                        # a last-bit softmax difference moved a candidate across the threshold
        assert diff.sum() <= 8 and (np.abs(p_prob[:, 1:][diff] - thres) < 1e-6).all()
    return same_head


def test_vgg_detect_matches_predict_at_600x1000(vgg):
    assert _detect_vs_predict(vgg, _frame(21, 600, 1000), 0.05, 21)          # 300 proposals = P: the head runs on the same rows


def test_fpn_detect_matches_predict_at_800x1344(fpn):
    _detect_vs_predict(fpn, _frame(23, 800, 1344), 0.02, 91)          # the threshold tests/test_gpu_model.py pins the FPN predict at


# ------------------------------------------------------------------------------------------------------------ 4. no host sync
def _host(det):
    return [t.clone() for t in det.to_host()]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_detect_captures_into_a_graph(fpn):
    """A host sync inside FRCNN.detect would raise during capture."""
    x = _frame(31, 800, 1344).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fpn.detect(x, 0.05)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fpn.detect(x, 0.05)
    g.replay()
    assert _equal(_host(out), _host(fpn.detect(x, 0.05)))


def test_detect_graph_replays_equal_eager_detect(vgg):
    from faster_rcnn_pytorch_amd.inference import DetectGraph
    H, W = 600, 1000
    xa, xb = _frame(41, H, W), _frame(42, H, W)
    ea, eb = _host(vgg.detect(xa.to(DEV), 0.05)), _host(vgg.detect(xb.to(DEV), 0.05))
    assert not _equal(ea, eb) and len(ea[1]) > 0 and len(eb[1]) > 0
    dg = DetectGraph(vgg, (H, W), threshold=0.05)
    ra = _host(dg(xa.to(DEV)))
    rb = _host(dg(xb.to(DEV)))
    ra2 = _host(dg(xa.to(DEV)))
    rb2 = _host(dg(xb.to(DEV)))
    assert _equal(ra, ea) and _equal(rb, eb) and _equal(ra2, ra) and _equal(rb2, rb)
    dg.set_threshold(0.2)                        # the threshold is read at replay time, not frozen into the graph
    r2 = _host(dg(xa.to(DEV)))
    e2 = _host(vgg.detect(xa.to(DEV), 0.2))
    assert _equal(r2, e2) and len(r2[1]) < len(ea[1])
