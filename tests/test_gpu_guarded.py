"""Where the hand-written ops touch memory (tests/guarded.py): every op family at its smallest hard shape, run under guarded(0xFF) and
again under guarded(0x00) with every operand, output and scratch buffer between two 256 KiB guards and every workspace at exactly
the size the op asked for.  Per case:
  (a) every guard byte is intact in both runs, the control words an op documents as "left zero" are zero, and every output lives in an
      arena (the exit checks of guarded());
  (b) the two runs agree bit for bit on the DEFINED part of every output -- the case names that part where a device count bounds it --
      so no result depends on bytes outside the operands or on what an output or the scratch held before;
  (c) the 0xFF run equals the op's reference, the one its own test file uses, with that file's exactness (named next to each check).

NOT_BIT_REPRODUCIBLE names the outputs that are compared under (c) only, with the reason.  Buffers in a library-private layout that is
padded to whole tiles (the conv stage's transformed activations / gradients / weights and its sign words) are declared -- they must
live in arenas and their guards are checked -- but compared through what their consumers compute from them.

DeviceSGD and the gradient norm are not here: tests/test_gpu_sgd.py and test_gpu_grad_clip.py run them on poisoned, oversized tables."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded as G
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

NOT_BIT_REPRODUCIBLE = {
    # include/frcnn_hip.h promises "bit-reproducible run to run" for frcnn_roi_pool_bwd_a16 only; the int32 entry point adds with fp32
    # atomics (LDS, and global ones on large bin grids) and documents no order
    "roi_pool int32 backward: grad_feat": "frcnn_roi_pool_bwd adds with fp32 atomics and documents no summation order",
    # csrc/roi_pool.hip roi_pool_bwd_launch: the wave-private planes (non-atomic adds) serve the 16-bit pair "wherever C is even"; an odd C takes
    # "the shared-plane form (LDS atomics, arrival order)"
    "roi_pool 16-bit backward at odd C: grad_feat": "the shared-plane kernel adds with LDS fp32 atomics in arrival order",
}


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


@pytest.fixture(scope="module")
def TF():
    from faster_rcnn_pytorch_amd import transforms
    return transforms


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rand_boxes(rng, n, lo=0.02, hi=0.6):
    c = rng.rand(n, 2) * 0.8 + 0.1
    wh = rng.rand(n, 2) * (hi - lo) + lo
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


def both(case, **kw):
    """(a) + (b); returns the 0xFF run's outputs for (c)."""
    return G.run_both(case, **kw)[0]


def close(got, ref, tol, scale_floor=1.0):
    """the existing tests' form: max |got - ref| < tol * max(scale_floor, max |ref|), ref in float64"""
    got, ref = got.double().cpu(), ref.double().cpu()
    err, scale = float((got - ref).abs().max()), max(scale_floor, float(ref.abs().max()))
    assert got.shape == ref.shape and err < tol * scale, (err, tol * scale)


# ============================================================================================ anchors, codec, IoU, prologue
@pytest.mark.parametrize("hw", [(16, 16), (37, 50), (112, 208)])       # 9 anchors (less than a wave), 54, 819 (several workgroups, a partial last one)
def test_anchor_grid(ops, hw):
    H, W = hw
    base = ops.anchor_base()
    out = both(lambda g: {"anchors": ops.anchor_grid([(H // 16, W // 16)], [(16, 16)], base[None], W, H, DEV)})
    assert np.array_equal(N(out["anchors"]), orc.anchor_grid(H, W))                       # (c) oracle, bit for bit


@pytest.mark.parametrize("n", [1, 65, 777])
def test_box_codec(ops, n):
    rng = np.random.RandomState(n)
    xy, anc_xy = rand_boxes(rng, n), rand_boxes(rng, n, 0.05, 0.5)
    cxcy, anc = orc.xy_to_cxcy(xy), orc.xy_to_cxcy(anc_xy)
    t = (rng.randn(n, 4) * np.array([0.5, 0.5, 0.3, 0.3])).astype(np.float32)

    def case(g):
        a, b, c, d = g.place(T(xy)), g.place(T(cxcy)), g.place(T(t)), g.place(T(anc))
        return {"xy_to_cxcy": ops.xy_to_cxcy(a), "cxcy_to_xy": ops.cxcy_to_xy(b), "decode": ops.decode(c, d), "encode": ops.encode(b, d)}
    out = both(case)
    assert np.array_equal(N(out["xy_to_cxcy"]), cxcy) and np.array_equal(N(out["cxcy_to_xy"]), orc.cxcy_to_xy(cxcy))     # (c) oracle, bit for bit
    assert np.array_equal(N(out["decode"]), orc.decode(t, anc), equal_nan=True)                                             # (c) oracle, bit for bit
    enc, enc_o = N(out["encode"]), orc.encode(cxcy, anc)
    assert np.array_equal(enc[:, :2], enc_o[:, :2]) and np.abs(enc[:, 2:] - enc_o[:, 2:]).max() < 1e-6                    # (c) logf columns: 1e-6, as test_codec_vs_oracle_and_golden


@pytest.mark.parametrize("n1,n2", [(65, 3), (777, 1), (1, 1)])
def test_pairwise_iou(ops, n1, n2):
    rng = np.random.RandomState(n1 + n2)
    a, b = rand_boxes(rng, n1), rand_boxes(rng, n2)
    out = both(lambda g: {"iou": ops.find_jaccard_overlap(g.place(T(a)), g.place(T(b)))})
    assert np.array_equal(N(out["iou"]), orc.pairwise_iou(a, b, 1e-5))                    # (c) oracle, bit for bit


@pytest.mark.parametrize("n", [1, 65, 777])
def test_proposal_prologue(ops, n):
    rng = np.random.RandomState(n + 1)
    anchor = orc.anchor_grid(600, 1000)
    anchor = np.ascontiguousarray(anchor[7::len(anchor) // n][:n])
    reg = (rng.randn(n, 4) * np.array([0.1, 0.1, 0.2, 0.2])).astype(np.float32)
    cls = np.stack([np.zeros(n, np.float32), (rng.randn(n) * 2 - 2).astype(np.float32)], 1)
    reg[::5, 2:] = -12.0                                  # boxes below min_size: score -1
    reg[n // 2, 2] = 120.0                                # exp overflow -> inf -> clamp

    def case(g):
        b, s = ops.proposal_prologue(g.place(T(reg)), g.place(T(cls)), g.place(T(anchor)), 1 / 1000)
        return {"boxes": b, "scores": s}
    out = both(case)
    b_o, s_o, _ = orc.proposal_prologue(reg, cls, anchor, 1 / 1000)
    assert np.array_equal(N(out["boxes"]), b_o, equal_nan=True) and np.array_equal(N(out["scores"]), s_o)     # (c) oracle, bit for bit


# ============================================================================================ top-k, NMS, region proposal
@pytest.mark.parametrize("n,k", [(1, 1), (65, 64), (777, 2000), (20646, 6000)])
@pytest.mark.parametrize("with_boxes", [True, False])
def test_topk_sorted(ops, n, k, with_boxes):
    """Defined part: the first count[0] entries of idx / scores / boxes (the rest of the K slots is not written when fewer than K scores
    are live)."""
    rng = np.random.RandomState(n + k)
    s = rng.rand(n).astype(np.float32)
    s[rng.rand(n) < 0.1] = -1.0
    if n == 1:
        s[0] = 0.5
    boxes = rand_boxes(rng, n)

    def case(g):
        idx, sc, bx, cnt = ops.topk_sorted(g.place(T(s)), k, g.place(T(boxes)) if with_boxes else None)
        m = int(cnt.item())
        return {"count": cnt, "idx": idx[:m], "scores": sc[:m], "boxes": bx[:m] if with_boxes else None}
    out = both(case)
    idx_o, sc_o = orc.topk_sorted(s, k)
    assert int(out["count"].item()) == len(idx_o) and np.array_equal(N(out["idx"]), idx_o) and np.array_equal(N(out["scores"]), sc_o)   # (c) oracle, bit for bit
    if with_boxes:
        assert np.array_equal(N(out["boxes"]), boxes[idx_o])


@pytest.mark.parametrize("k,thr", [(3, 0.5), (65, 0.5), (777, 0.5), (2049, 0.7), (16385, 0.7)])     # 2049: one box past the top level's 2048; 16385: one past NMS_CASCADE_MIN
def test_nms_sorted(ops, k, thr):
    """Defined part: the first count[0] rows of keep and rois."""
    rng = np.random.RandomState(k)
    c = rng.rand(k, 2).astype(np.float32) * 0.7 + 0.15
    wh = rng.rand(k, 2).astype(np.float32) * 0.25 + 0.03
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    live = max(1, k - 37)

    def case(g):
        keep, rois, cnt = ops.nms_sorted(g.place(T(b)), thr, want_rois=True)
        m = int(cnt.item())
        keep2, _, cnt2 = ops.nms_sorted(g.place(T(b)), thr, n_boxes=g.place(T(np.array([live], np.int32))))       # a device-side live count
        m2 = int(cnt2.item())
        return {"count": cnt, "keep": keep[:m], "rois": rois[:m], "count_live": cnt2, "keep_live": keep2[:m2]}
    out = both(case)
    ko, kl = orc.nms(b, thr), orc.nms(b[:live], thr)
    assert int(out["count"].item()) == len(ko) and np.array_equal(N(out["keep"]), ko) and np.array_equal(N(out["rois"]), b[ko])     # (c) oracle, bit for bit
    assert int(out["count_live"].item()) == len(kl) and np.array_equal(N(out["keep_live"]), kl)


@pytest.mark.parametrize("n,ncls", [(3, 2), (777, 5), (2049, 20)])
def test_batched_nms(ops, n, ncls):
    """batched_nms returns order[keep[:count]], a gather torch makes, so the result is compared as values (derived) and the buffers the
    kernels write -- keep [n] and the count [1], allocated in ops.batched_nms, and the sorted idx / scores / boxes / count of ops.topk_sorted
    -- are asserted to be arenas by g.expect_arenas."""
    rng = np.random.RandomState(n)
    b = rand_boxes(rng, n, 0.05, 0.4)
    sc = ((rng.permutation(n) + 1) / np.float32(n + 1)).astype(np.float32)
    cl = rng.randint(0, ncls, n).astype(np.int64)
    def case(g):
        kept = ops.batched_nms(g.place(T(b)), g.place(T(sc)), g.place(T(cl)), 0.3)
        g.expect_arenas("batched_nms", [(n,), (1,)])
        g.expect_arenas("topk_sorted", [(n,), (n,), (n, 4), (1,)])
        return {"kept_indices": kept}
    res = G.run_both(case, derived=("kept_indices",))[0]
    exp = np.concatenate([np.nonzero(cl == q)[0][orc.nms(b[cl == q], 0.3, order=np.argsort(-sc[cl == q], kind="stable"))] for q in range(ncls)])
    exp = exp[np.argsort(-sc[exp], kind="stable")]
    assert np.array_equal(N(res["kept_indices"]), exp)                                    # (c) the oracle's per-class loop, bit for bit (test_nms_cascade_keep_lists_vs_oracle)


@pytest.mark.parametrize("hw,pre,post", [((16, 16), 3000, 300), ((64, 112), 64, 20), ((160, 240), 3000, 300)])       # N = 9, 252, 1350 anchors
@pytest.mark.parametrize("anchors_from", ["hbm", "registers"])
def test_region_proposal(ops, hw, pre, post, anchors_from):
    """Defined part: rois[:count] and src[:count]; the rows of rois behind the count are zeros (torch.zeros in the op) and compared too."""
    H, W = hw
    rng = np.random.RandomState(H + W)
    anchor = orc.anchor_grid(H, W)
    n = anchor.shape[0]
    reg = (rng.randn(n, 4) * np.array([0.1, 0.1, 0.2, 0.2])).astype(np.float32)
    cls = np.stack([np.zeros(n, np.float32), (rng.randn(n) * 2 - 2).astype(np.float32)], 1)
    grid = (H // 16, W // 16, 16, ops.anchor_base(), W, H)

    def case(g):
        a = g.place(T(anchor)) if anchors_from == "hbm" else None
        rois, cnt, src = ops.region_proposal(g.place(T(reg)), g.place(T(cls)), a, 1 / 1000, pre, 0.7, post, grid=None if a is not None else grid, want_src=True)
        m = int(cnt.item())
        return {"count": cnt, "rois": rois[:m], "src": src[:m], "rois_tail": rois[m:]}
    out = both(case)
    rois_o, src_o = orc.region_proposal(reg, cls, anchor, 1 / 1000, min(pre, n), 0.7, post)
    assert int(out["count"].item()) == len(rois_o) and np.array_equal(N(out["src"]), src_o) and np.array_equal(N(out["rois"]), rois_o)    # (c) oracle, bit for bit
    assert not N(out["rois_tail"]).any()


# ============================================================================================ target makers
import targets_ref as tr                                      # noqa: E402
import test_gpu_targets_exact as tgx                          # noqa: E402  (its checks against tests/targets_ref.py, used as they are)
from oracle import philox_ref                                 # noqa: E402

# the small exact cases of test_gpu_targets_exact.py: one anchor; both sides of a wave; G = 1 on 2600 anchors (several workgroups); the
# sampled form one past the 1024-anchor block; more ground truths than one 64-wide pass
RPN_CASES = ["N1-v0", "N65-v0", "N257-v1", "G1-v1", "G65-v0", "N1025-sampled-v0", "thresholds-v1"]
HEAD_CASES = ["thresholds-v0", "argmax-ties-v1", "device-count-v0", "n1025-phase1-v1", "quota-v0-pos+1-neg-1"]


@pytest.mark.parametrize("name", RPN_CASES)
@pytest.mark.parametrize("mode", ["host_perms", "device_rng", "device_rng_state"])
def test_rpn_targets(ops, name, mode):
    """Every row of cls / reg and the four counts are defined.  device_rng_state: (seed, offset) come from a device tensor that the call
    advances -- an output too.  (c) tests/targets_ref.py through test_gpu_targets_exact._check_rpn: labels, counts and the two linear
    columns bit for bit, the log columns within 1e-6 of float64."""
    c = tr.rpn_case(name)
    pp, pn = tgx._host_perms(c)

    def case(g):
        a, gt = g.place(T(tr.to_f32(c.anchors))), g.place(T(tr.to_f32(c.gt)))
        if mode == "host_perms":
            cls, reg, counts = ops.rpn_targets(a, gt, variant=c.variant, perm_pos=g.place(T(pp, torch.int64)), perm_neg=g.place(T(pn, torch.int64)))
            return {"cls": cls, "reg": reg, "counts": counts}
        if mode == "device_rng":
            cls, reg, counts = ops.rpn_targets(a, gt, variant=c.variant, seed=tgx.SEED, offset=tgx.OFFSET)
            return {"cls": cls, "reg": reg, "counts": counts}
        st = g.place(ops.philox_state(tgx.SEED, tgx.OFFSET, DEV))
        cls, reg, counts = ops.rpn_targets(a, gt, variant=c.variant, philox_state=st)
        return {"cls": cls, "reg": reg, "counts": counts, "philox_state": st}
    out = both(case)
    want = tr.rpn_sample(c, pp, pn) if mode == "host_perms" else tgx._philox_labels(c, tgx.SEED, tgx.OFFSET)
    tgx._check_rpn(c, N(out["cls"]), N(out["reg"]), N(out["counts"]).tolist(), want, mode)
    if mode == "device_rng_state":
        assert N(out["philox_state"]).tolist() == N(ops.philox_state(tgx.SEED, tgx.OFFSET + 1, "cpu")).tolist()


@pytest.mark.parametrize("name", HEAD_CASES)
@pytest.mark.parametrize("mode", ["host_perms", "device_rng", "device_rng_state"])
def test_head_targets(ops, name, mode):
    """All `total` rows of cls / reg / sample_rois / keep are defined (rows that could not be sampled: -1 and zeros).  device_rng_state:
    (seed, offset) come from a device tensor that the call advances -- an output too.  (c)
    tests/targets_ref.py through test_gpu_targets_exact._check_head: everything bit for bit, the log columns within 1e-5."""
    c = tr.head_case(name)
    r = tr.head_match(c)
    if mode == "host_perms":
        pp, pn = tr.head_perms(c, "random")
    else:
        pp, pn = philox_ref.sampling_perm(tgx.SEED, tgx.OFFSET, 2, r.pos_list), philox_ref.sampling_perm(tgx.SEED, tgx.OFFSET, 3, r.neg_list)

    def case(g):
        n_rois = g.place(T(np.array([c.n_rois], np.int32))) if c.n_rois != c.rois.shape[0] else None
        st = g.place(ops.philox_state(tgx.SEED, tgx.OFFSET, DEV)) if mode == "device_rng_state" else None
        kw = dict(perm_pos=g.place(T(pp, torch.int64)), perm_neg=g.place(T(pn, torch.int64))) if mode == "host_perms" else \
            dict(seed=tgx.SEED, offset=tgx.OFFSET) if mode == "device_rng" else dict(philox_state=st)
        cls, reg, srois, keep, counts = ops.head_targets(g.place(T(c.rois_f32())), g.place(T(tr.to_f32(c.gt))), g.place(T(c.gt_label)), n_rois=n_rois, variant=c.variant,
                                                         label_offset=c.label_offset, max_pos=c.max_pos, total=c.total, want_keep=True, **kw)
        return {"cls": cls, "reg": reg, "sample_rois": srois, "keep": keep, "counts": counts, "philox_state": st}
    out = both(case)
    tgx._check_head(c, [out[k] for k in ("cls", "reg", "sample_rois", "keep", "counts")], pp, pn, mode)
    if mode == "device_rng_state":
        assert N(out["philox_state"]).tolist() == N(ops.philox_state(tgx.SEED, tgx.OFFSET + 1, "cpu")).tolist()


# ============================================================================================ RoI ops
def _pool_inputs(C_, H, W, R):
    rng = np.random.RandomState(C_ + R)
    f = rng.randn(C_, H, W).astype(np.float32)
    rois = rand_boxes(rng, R, 0.02, 0.9) * np.array([W, H, W, H], np.float32)
    rois[0] = [0, 0, W, H]
    rois[1] = [W * 0.5, H * 0.5, W * 0.5, H * 0.5]
    rois[2] = [W + 3, H + 3, W + 9, H + 9]                    # outside: empty bins
    return rng, f, rois


@pytest.mark.parametrize("C_,H,W,R", [(3, 9, 11, 5), (6, 9, 11, 5), (64, 50, 50, 17)])
@pytest.mark.parametrize("argmax", ["16-bit", "int32"])
def test_roi_pool(ops, C_, H, W, R, argmax):
    """Through autograd, as the model calls it: 7 x 7 bins on these planes take the library-private 16-bit argmax pair, any other bin
    grid (5 x 5 here) the int32 pair.  (c) the oracle: pooled values bit for bit, gradient within 1e-5 (another fp32 order), as
    test_roi_pool_fwd_bwd_vs_oracle."""
    PH = 7 if argmax == "16-bit" else 5
    rng, f, rois = _pool_inputs(C_, H, W, R)
    out_o, arg_o = orc.roi_pool_fwd(f, rois, PH, PH, 1.0)
    go = rng.randn(*out_o.shape).astype(np.float32)

    def case(g):
        ft = g.place(T(f[None]).requires_grad_(True))
        out = ops.roi_pool(ft, g.place(T(rois)), (PH, PH), 1.0)
        (gf,) = torch.autograd.grad(out, ft, g.place(T(go)))
        return {"out": out, "grad_feat": gf}
    out = both(case, only_reference=("grad_feat",) if argmax == "int32" or C_ % 2 else ())          # the two entries of NOT_BIT_REPRODUCIBLE
    assert np.array_equal(N(out["out"]), out_o)
    assert np.allclose(N(out["grad_feat"])[0], orc.roi_pool_bwd(go, arg_o, C_, H, W), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("C_,H,W,R", [(3, 9, 11, 5), (6, 9, 11, 5), (64, 50, 50, 17)])
def test_roi_pool_with_int32_argmax(ops, C_, H, W, R):
    """The torchvision-shaped forward: values AND argmax (-1 = empty bin) bit for bit vs the oracle (test_roi_pool_int32_argmax_abi_bit_exact)."""
    _, f, rois = _pool_inputs(C_, H, W, R)

    def case(g):
        out, arg = ops.roi_pool_with_argmax(g.place(T(f[None])), g.place(T(rois)), (7, 7), 1.0)
        return {"out": out, "argmax": arg}
    out = both(case)
    out_o, arg_o = orc.roi_pool_fwd(f, rois, 7, 7, 1.0)
    assert np.array_equal(N(out["out"]), out_o) and np.array_equal(N(out["argmax"]), arg_o) and (arg_o[2] == -1).all()


@pytest.mark.parametrize("R", [1, 65, 300])
def test_roi_level_map_and_scale_order(ops, R):
    """roi_level_map vs the oracle bit for bit; roi_scale_order: the scaled boxes are torch's own fp32 products bit for bit, `order` is the
    permutation that sorts the cost keys descending with ties by index (test_roi_scale_order_and_ordered_forward_are_bit_identical)."""
    rng = np.random.RandomState(R)
    Hh, Ww = 800, 1344
    shapes, scales = [(200, 336), (100, 168), (50, 84), (25, 42)], (0.25, 0.125, 0.0625, 0.03125)
    b = rand_boxes(rng, R, 0.01, 0.9)
    sq = np.array([[0, 0, s, s] for s in (50, 111.9, 112, 223.9, 224, 447.9, 448, 895, 896, 2000, 0)], np.float32)[:R]
    px = (b * np.array([Ww, Hh, Ww, Hh], np.float32)).astype(np.float32)
    px[:len(sq)] = sq
    mul = np.array([Ww, Hh, Ww, Hh], np.float32)

    def case(g):
        scaled, order, cost = ops.roi_scale_order(g.place(T(b)), mul, shapes, scales, want_cost=True)
        return {"levels": ops.roi_level_map(g.place(T(px))), "scaled": scaled, "order": order, "cost": cost}
    out = both(case)
    assert np.array_equal(N(out["levels"]), orc.roi_level_map(px))
    assert torch.equal(out["scaled"], T(b) * T(mul))
    o, c = N(out["order"]).astype(np.int64), N(out["cost"]).astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(o, np.lexsort((np.arange(R), -c)))


def test_ms_roi_align_forward_and_backward_vs_oracle(ops):
    """Four levels of a 672 x 400 frame, C = 16, 60 RoIs with two that stick out of the frame (the forward's clamped taps at the map edge):
    (c) the oracle, forward within 1e-5 and gradients within 1e-4, as test_ms_roi_align_fwd_bwd_vs_oracle."""
    rng = np.random.RandomState(1)
    C_ = 16
    shapes = [(100, 168), (50, 84), (25, 42), (13, 21)]
    feats = [rng.randn(C_, h, w).astype(np.float32) for h, w in shapes]
    rois = rand_boxes(rng, 60, 0.02, 0.9) * np.array([672, 400, 672, 400], np.float32)
    rois[0] = [-20, -10, 100, 90]
    rois[1] = [600, 350, 700, 420]
    out_o, lv = orc.ms_roi_align(feats, rois)
    go = rng.randn(*out_o.shape).astype(np.float32)

    def case(g):
        fts = [g.place(T(f[None]).requires_grad_(True)) for f in feats]
        out = ops.ms_roi_align(fts, g.place(T(rois)), 7, 2)
        grads = torch.autograd.grad(out, fts, g.place(T(go)))
        return dict({"out": out}, **{"grad_level%d" % l: t for l, t in enumerate(grads)})
    out = both(case)
    assert np.abs(N(out["out"]) - out_o).max() < 1e-5
    for l in range(4):
        ref = orc.roi_align_bwd(go, feats[l].shape, rois, 0.25 / (1 << l), 2, False, lv, l)
        assert np.allclose(N(out["grad_level%d" % l])[0], ref, rtol=1e-4, atol=1e-4)


import roi_align_ref as ra                                    # noqa: E402


# regC:3 / regC:33: the register path with a partial channel group; seg:33: two segments through the workspace; mixed: RoIs with 1 KB
# records and RoIs whose weight tables are built inside the tile kernel, in the same lists, on the LDS-DMA path; generic:4/2: the
# memset + atomics kernel (exact data: every order gives the same bits); shape:1x3: a level smaller than a tile
@pytest.mark.parametrize("name", ["regC:3", "regC:33", "seg:33", "mixed:", "generic:4/2", "shape:1x3"])
def test_ms_roi_align_backward_on_exact_data(ops, name):
    """(c) float64 on exact data, bit for bit (test_gpu_roi_align_exact.py, through autograd)."""
    c = ra.case(name)

    def case(g):
        fts = [g.place(torch.zeros((1, c.C, h, w), device=DEV).requires_grad_(True)) for h, w in c.shapes]
        out = ops.ms_roi_align(fts, g.place(T(c.rois)), c.PH, c.SR, scales=c.scales, aligned=c.aligned)
        grads = torch.autograd.grad(out, fts, g.place(T(c.go)))
        return {"grad_level%d" % l: t for l, t in enumerate(grads)}
    out = both(case)
    for l, (gref, _) in enumerate(ra.case_ref(name)):
        assert np.array_equal(bits32(N(out["grad_level%d" % l])[0]), bits32(np.asarray(gref).astype(np.float32))), (name, l)


# ============================================================================================ RPN head
def _head_params(g, C_, A):
    return [torch.randn(C_, generator=g) * 0.1, torch.randn(2 * A, C_, 1, 1, generator=g) * 0.02, torch.randn(2 * A, generator=g) * 0.1,
            torch.randn(4 * A, C_, 1, 1, generator=g) * 0.02, torch.randn(4 * A, generator=g) * 0.1]


def _head_ref64(raws, b3, wc, bc, wr, br):
    cc, rr = [], []
    for r in raws:
        h = torch.relu(r + b3[None, :, None, None])
        cc.append(F.conv2d(h, wc, bc).permute(0, 2, 3, 1).contiguous().view(1, -1, 2))
        rr.append(F.conv2d(h, wr, br).permute(0, 2, 3, 1).contiguous().view(1, -1, 4))
    return torch.cat(cc, 1), torch.cat(rr, 1)


def test_rpn_head_tail_forward_at_the_small_width(ops):
    """(64, 5, 7, A = 9): 35 positions, less than one MFMA tile; forward only (the fused backward is built for C = 256 / 512).
    (c) float64 of the op chain within 1e-5 absolute (test_rpn_head_tail_vs_torch_fp32)."""
    g0 = torch.Generator().manual_seed(64 + 9)
    raw = torch.randn(1, 64, 5, 7, generator=g0)
    params = _head_params(g0, 64, 9)
    out = both(lambda g: dict(zip(("cls", "reg"), ops.rpn_head_tail(g.place(raw.to(DEV)), *[g.place(p.to(DEV)) for p in params]))))
    ref_c, ref_r = _head_ref64([raw.double()], *[p.double() for p in params])
    assert float((out["cls"].cpu().double() - ref_c).abs().max()) < 1e-5 and float((out["reg"].cpu().double() - ref_r).abs().max()) < 1e-5


# [(9, 33)]: 297 positions, odd width; [(3, 4)]: 12 positions; [(70, 130), (5, 64)]: two levels, the second starting inside a tile
@pytest.mark.parametrize("shapes", [[(9, 33)], [(3, 4)], [(70, 130), (5, 64)]], ids=["9x33", "3x4", "70x130+5x64"])
@pytest.mark.parametrize("dtype,mfma,tol", [("f32", "f32", 1e-5), ("bf16", "bf16", 2e-2)])
def test_rpn_head_tail_levels_forward_and_backward(ops, shapes, dtype, mfma, tol):
    """C = 256, A = 3: all levels in one launch, forward and the fused backward.  (c) float64 of the op chain on the same (bf16-rounded)
    conv outputs: forward `tol` absolute; gradients 2e-4 (f32) / 1e-2 (bf16) of the scale (test_rpn_head_tail_all_fpn_levels_one_launch)."""
    g0 = torch.Generator().manual_seed(11)
    C_, A = 256, 3
    raws = [torch.randn(1, C_, h, w, generator=g0) for h, w in shapes]
    if dtype == "bf16":
        raws = [r.bfloat16() for r in raws]
    params = _head_params(g0, C_, A)
    n = sum(h * w for h, w in shapes) * A
    gc, gr = torch.randn(1, n, 2, generator=g0), torch.randn(1, n, 4, generator=g0)
    names = ["d_raw%d" % l for l in range(len(raws))] + ["d_b3", "d_w_cls", "d_b_cls", "d_w_reg", "d_b_reg"]

    def case(g):
        dr = [g.place(r.to(DEV).requires_grad_(True)) for r in raws]
        ps = [g.place(p.to(DEV).requires_grad_(True)) for p in params]
        cls, reg = ops.rpn_head_tail_levels(dr, *ps, mfma=mfma)
        grads = torch.autograd.grad([cls, reg], dr + ps, [g.place(gc.to(DEV)), g.place(gr.to(DEV))])
        return dict({"cls": cls, "reg": reg}, **dict(zip(names, grads)))
    out = both(case)                                          # (d_w_cls / d_w_reg: the kernel writes [n, C]; autograd hands back the [n, C, 1, 1] view of the same buffer)
    ref_in = [r.double().requires_grad_(True) for r in raws] + [p.clone().double().requires_grad_(True) for p in params]
    ref_c, ref_r = _head_ref64(ref_in[:len(raws)], *ref_in[len(raws):])
    assert float((out["cls"].cpu().double() - ref_c.detach()).abs().max()) < tol and float((out["reg"].cpu().double() - ref_r.detach()).abs().max()) < tol
    ((ref_c * gc.double()).sum() + (ref_r * gr.double()).sum()).backward()
    btol = 2e-4 if dtype == "f32" else 1e-2
    for k, b in zip(names, ref_in):
        close(out[k], b.grad, btol)


@pytest.mark.parametrize("shapes", [[(9, 33)], [(3, 4)], [(70, 130), (5, 64)]], ids=["9x33", "3x4", "70x130+5x64"])
def test_rpn_conv_head_levels_bf16(ops, shapes):
    """The fused bf16 RPN head (csrc/rpn_conv.hip): forward, and its three backward kernels through autograd.  (c) float64 on the same
    bf16-rounded operands with the tolerances of test_rpn_conv_head_bf16_vs_torch / _bwd_data_ / _wgrad_bf16_vs_torch: cls / reg 2e-2
    absolute; data gradients 3e-2 of the scale; b3 8e-2, the 1 x 1 parameters 3e-2 of their largest gradient.  The 3 x 3 weight gradient
    is held to float64 by the stand-alone call below (1e-3), where its operand d_raw is given."""
    g0 = torch.Generator().manual_seed(21)
    C_, A = 256, 3
    feats = [torch.randn(1, C_, h, w, generator=g0).bfloat16() for h, w in shapes]
    ps = [torch.randn(C_, C_, 3, 3, generator=g0) * 0.01] + _head_params(g0, C_, A)
    n = sum(h * w for h, w in shapes) * A
    gc, gr = torch.randn(1, n, 2, generator=g0), torch.randn(1, n, 4, generator=g0)
    names = ["d_feat%d" % l for l in range(len(feats))] + ["d_w3", "d_b3", "d_w_cls", "d_b_cls", "d_w_reg", "d_b_reg"]

    def case(g):
        fin = [g.place(f.to(DEV).requires_grad_(True)) for f in feats]
        pd = [g.place(p.to(DEV).requires_grad_(True)) for p in ps]
        cls, reg = ops.rpn_conv_head_levels(fin, *pd)
        grads = torch.autograd.grad([cls, reg], fin + pd, [g.place(gc.to(DEV)), g.place(gr.to(DEV))])
        return dict({"cls": cls, "reg": reg}, **dict(zip(names, grads)))
    out = both(case)
    rin = [f.double().requires_grad_(True) for f in feats]
    rp = [t.clone().double().requires_grad_(True) for t in (ps[0].bfloat16().double(), ps[1], ps[2].bfloat16().float(), ps[3], ps[4].bfloat16().float(), ps[5])]
    raws = [F.conv2d(f, rp[0], None, padding=1) for f in rin]
    ref_c, ref_r = _head_ref64(raws, *rp[1:])
    assert float((out["cls"].cpu().double() - ref_c.detach()).abs().max()) < 2e-2 and float((out["reg"].cpu().double() - ref_r.detach()).abs().max()) < 2e-2
    ((ref_c * gc.double()).sum() + (ref_r * gr.double()).sum()).backward()
    for l, b in enumerate(rin):
        close(out["d_feat%d" % l], b.grad, 3e-2)
    for i, (k, b) in enumerate(zip(names[len(feats):], rp)):
        if i == 0:
            continue
        close(out[k], b.grad, 8e-2 if i == 1 else 3e-2, scale_floor=1e-3)


@pytest.mark.parametrize("shapes", [[(9, 33)], [(3, 4)], [(70, 130), (5, 64)]], ids=["9x33", "3x4", "70x130+5x64"])
def test_rpn_conv_bwd_data_and_wgrad_bf16(ops, shapes):
    """(c) float64 on the same bf16-rounded operands: data gradient 6e-3 of the scale (test_rpn_conv_bwd_data_bf16_vs_torch), weight gradient
    1e-3 of the largest entry (test_rpn_conv_wgrad_bf16_vs_torch)."""
    g0 = torch.Generator().manual_seed(44)
    feats = [torch.randn(1, 256, h, w, generator=g0).bfloat16() for h, w in shapes]
    d_raws = [(torch.randn(1, 256, h, w, generator=g0) * 0.1).bfloat16() for h, w in shapes]
    w3 = torch.randn(256, 256, 3, 3, generator=g0) * 0.01

    def case(g):
        fd, dd = [g.place(f.to(DEV)) for f in feats], [g.place(d.to(DEV)) for d in d_raws]
        dxs = ops.rpn_conv_bwd_data(dd, g.place(w3.to(DEV)))
        return dict({"dw3": ops.rpn_conv_wgrad(fd, dd)}, **{"d_feat%d" % l: t for l, t in enumerate(dxs)})
    out = both(case)
    for l, d in enumerate(d_raws):
        ref = F.conv_transpose2d(d.double(), w3.bfloat16().double(), padding=1)
        assert out["d_feat%d" % l].dtype == torch.bfloat16
        close(out["d_feat%d" % l], ref, 6e-3)
    w = torch.zeros(256, 256, 3, 3, dtype=torch.float64, requires_grad=True)
    sum((F.conv2d(f.double(), w, None, padding=1) * d.double()).sum() for f, d in zip(feats, d_raws)).backward()
    err = float((out["dw3"].cpu().double() - w.grad).abs().max())
    assert err < 1e-3 * float(w.grad.abs().max()), err


# ============================================================================================ fp32 conv stage (csrc/rpn_conv_f32.hip)
@pytest.fixture(params=["native", "split"])
def products(request, ops):
    """both forms of the stage's products (ops.conv3x3_f32_products); the switch comes back as it was"""
    prev = ops.conv3x3_f32_products(request.param)
    yield request.param
    ops.conv3x3_f32_products(prev)


def test_rpn_conv3x3_f32(ops, products):
    """"odd", C = 128: rows and columns shorter than a strip, a single pixel, a wrap inside a fragment.  Every call gets a fresh, zeroed,
    exact-size control workspace.  (c) float64 on the CPU: forward and data gradient 2e-5 of the scale, weight gradient 1e-4
    (test_rpn_conv3x3_f32_forward_backward_vs_float64; the split products are held to the same bounds by
    test_conv3x3_f32_split_products_are_as_close_to_float64_as_the_native_ones)."""
    C_, shapes = 128, [(5, 7), (1, 1), (3, 130), (17, 2)]
    g0 = torch.Generator().manual_seed(3 + C_)
    feats = [torch.randn(1, C_, h, w, generator=g0) for h, w in shapes]
    wt = torch.randn(C_, C_, 3, 3, generator=g0) * (2.0 / (9 * C_)) ** 0.5
    gouts = [torch.randn(1, C_, h, w, generator=g0) for h, w in shapes]

    def case(g):
        fd, gd, wd = [g.place(f.to(DEV)) for f in feats], [g.place(t.to(DEV)) for t in gouts], g.place(wt.to(DEV))
        out = {"y%d" % l: t for l, t in enumerate(ops.rpn_conv3x3_fwd(fd, wd))}
        out.update({"dx%d" % l: t for l, t in enumerate(ops.rpn_conv3x3_bwd_data(gd, wd))})
        out["dw"] = ops.rpn_conv3x3_wgrad(fd, gd)
        return out
    out = both(case)
    wref = torch.zeros(C_, C_, 3, 3, dtype=torch.float64)
    for l, (f, t) in enumerate(zip(feats, gouts)):
        close(out["y%d" % l], F.conv2d(f.double(), wt.double(), None, padding=1), 2e-5)
        close(out["dx%d" % l], F.conv_transpose2d(t.double(), wt.double(), None, padding=1), 2e-5)
        wref += torch.nn.grad.conv2d_weight(f.double(), (C_, C_, 3, 3), t.double(), padding=1)
    close(out["dw"], wref, 1e-4)


CONV3X3 = [   # name, Cin, Cout, level shapes, bias, relu (the cases of test_conv3x3_f32_stage_vs_float64)
    ("levels", 128, 128, [(9, 14), (30, 5), (1, 1)], False, True),            # several levels sharing the weight, a single pixel, no bias
    ("narrow_both", 64, 64, [(20, 30), (7, 9)], True, True),                  # 64-wide tiles on both sides, F(2x2), odd sizes
    ("rpn_37x62", 256, 128, [(37, 62)], True, True),                          # 160 4 x 4 tiles padded to 192: a padded product tile
    ("wide_in", 384, 128, [(20, 31)], True, False),                           # bias without ReLU: no sign words
]


def _conv_data(name, Cin, Cout, shapes, use_bias):
    g0 = torch.Generator().manual_seed(len(name) * 7 + Cin)
    xs = [torch.randn(1, Cin, h, w, generator=g0) for h, w in shapes]
    wt = torch.randn(Cout, Cin, 3, 3, generator=g0) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g0) * 0.2 if use_bias else None
    dys = [torch.randn(1, Cout, h, w, generator=g0) for h, w in shapes]
    return xs, wt, b, dys


def _conv_check(out, xs, wt, b, dys, relu, keys=("y", "dx", "dw", "db")):
    """float64 on the CPU with the ReLU mask of the DEVICE output, as test_conv3x3_f32_stage_vs_float64: y and dx 2e-5, dw and db 1e-4 of the scale"""
    Cout, Cin = wt.shape[:2]
    pre = [F.conv2d(x.double(), wt.double(), None if b is None else b.double(), padding=1) for x in xs]
    for l, p in enumerate(pre):
        r = p.clamp_min(0) if relu else p
        assert float((out["y%d" % l].double().cpu() - r).abs().max()) < 2e-5 * max(1.0, float(p.abs().max()))
    masks = [(out["y%d" % l].cpu() > 0) for l in range(len(xs))] if relu else [torch.ones_like(p, dtype=torch.bool) for p in pre]
    gs = [t.double() * m for t, m in zip(dys, masks)]
    w_ref, b_ref = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64), torch.zeros(Cout, dtype=torch.float64)
    for l, (x, t) in enumerate(zip(xs, gs)):
        for k in [k for k in keys if k.startswith("dx")]:
            close(out["%s%d" % (k, l)], F.conv_transpose2d(t, wt.double(), None, padding=1), 2e-5)
        w_ref += torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), t, padding=1)
        b_ref += t.sum(dim=(0, 2, 3))
    for k in [k for k in keys if k.startswith("dw")]:
        close(out[k], w_ref, 1e-4)
    for k in [k for k in keys if k.startswith("db")]:
        close(out[k], b_ref, 1e-4)


@pytest.mark.parametrize("name,Cin,Cout,shapes,use_bias,relu", CONV3X3, ids=[c[0] for c in CONV3X3])
def test_conv3x3_f32_independent_calls(ops, products, name, Cin, Cout, shapes, use_bias, relu):
    """conv3x3_fwd (bias, ReLU + sign words, keep_transformed, u_rotated), conv3x3_bwd_data (sign words; the forward's rotated weights),
    conv3x3_wgrad (sign words, bias gradient; the forward's transformed activations): every call with a fresh zeroed control workspace of
    exactly frcnn_conv3x3_f32_workspace bytes.  x_transformed / u_rotated / the sign words are tile-padded private layouts: declared, and
    compared through dx_u and dw_x, which are computed from them."""
    xs, wt, b, dys = _conv_data(name, Cin, Cout, shapes, use_bias)

    def case(g):
        xd, dyd, wd = [g.place(x.to(DEV)) for x in xs], [g.place(t.to(DEV)) for t in dys], g.place(wt.to(DEV))
        bd = None if b is None else g.place(b.to(DEV))
        urot = ops.conv3x3_u_buffer(xd, wd)
        ys, xt, bits = ops.conv3x3_fwd(xd, wd, bd, relu, keep_transformed=True, want_bits=relu, u_rotated=urot)
        g.outputs(x_transformed=xt, relu_bits=bits, u_rotated=urot)
        out = {"y%d" % l: t for l, t in enumerate(ys)}
        out.update({"plain_y%d" % l: t for l, t in enumerate(ops.conv3x3_fwd(xd, wd, bd, relu))})
        out.update({"dx%d" % l: t for l, t in enumerate(ops.conv3x3_bwd_data(dyd, wd, bits))})
        out.update({"dx_u%d" % l: t for l, t in enumerate(ops.conv3x3_bwd_data(dyd, wd, bits, u_rotated=urot))})
        out["dw"], out["db"] = ops.conv3x3_wgrad(xd, dyd, bits, want_bias=True)
        out["dw_x"], out["db_x"] = ops.conv3x3_wgrad(xd, dyd, bits, want_bias=True, x_transformed=xt)
        return out
    out = both(case)
    _conv_check(out, xs, wt, b, dys, relu, keys=("y", "dx", "dx_u", "dw", "dw_x", "db", "db_x"))
    for l in range(len(xs)):                                  # with or without the extras: the same bits (test_conv3x3_f32_stage_vs_float64)
        assert torch.equal(out["y%d" % l], out["plain_y%d" % l]) and torch.equal(out["dx%d" % l], out["dx_u%d" % l])
    assert torch.equal(out["dw"], out["dw_x"]) and torch.equal(out["db"], out["db_x"])


@pytest.mark.parametrize("name,Cin,Cout,shapes,use_bias,relu", CONV3X3[:3], ids=[c[0] for c in CONV3X3[:3]])
def test_conv3x3_f32_staged_gradient_pair_and_the_one_call_backward(ops, products, name, Cin, Cout, shapes, use_bias, relu):
    """conv3x3_bwd_data(dy_transformed=, want_bias_partials=True) leaves the bias gradient's partial sums IN THE CONTROL WORKSPACE for the
    conv3x3_wgrad(dy_transformed=) "called NEXT on the same workspace" (include/frcnn_hip.h): these two calls, and only they, share ONE
    arena (g.sharing_ctrl).  The forward before them and conv3x3_bwd -- the same pair in one call -- each get a fresh, zeroed, exact-size one."""
    xs, wt, b, dys = _conv_data(name, Cin, Cout, shapes, use_bias)

    def case(g):
        xd, dyd, wd = [g.place(x.to(DEV)) for x in xs], [g.place(t.to(DEV)) for t in dys], g.place(wt.to(DEV))
        bd = None if b is None else g.place(b.to(DEV))
        ys, xt, bits = ops.conv3x3_fwd(xd, wd, bd, relu, keep_transformed=True, want_bits=relu)
        dyt = ops.conv3x3_dy_buffer(shapes, Cout, DEV)
        g.outputs(x_transformed=xt, relu_bits=bits, dy_transformed=dyt)
        out = {"y%d" % l: t for l, t in enumerate(ys)}
        with g.sharing_ctrl("rpn_conv_f32"):                  # the bias partials travel in the workspace from the first call to the second
            out.update({"dx%d" % l: t for l, t in enumerate(ops.conv3x3_bwd_data(dyd, wd, bits, dy_transformed=dyt, want_bias_partials=True))})
            out["dw"], out["db"] = ops.conv3x3_wgrad(xd, dyd, bits, want_bias=True, x_transformed=xt, dy_transformed=dyt)
        dxs, out["dw_one"], out["db_one"] = ops.conv3x3_bwd(dyd, wd, xt, bits, want_bias=True)
        out.update({"dx_one%d" % l: t for l, t in enumerate(dxs)})
        return out
    out = both(case)
    _conv_check(out, xs, wt, b, dys, relu, keys=("y", "dx", "dx_one", "dw", "dw_one", "db", "db_one"))
    for l in range(len(xs)):                                  # "bit for bit conv3x3_bwd_data(..., dy_transformed=) followed by conv3x3_wgrad" (ops.conv3x3_bwd)
        assert torch.equal(out["dx%d" % l], out["dx_one%d" % l])
    assert torch.equal(out["dw"], out["dw_one"]) and torch.equal(out["db"], out["db_one"])


def test_conv3x3_f32_fused_relu_maxpool(ops, products):
    """64 -> 128 on 75 x 125: odd rows and columns, so the last row and column of the map belong to no 2 x 2 window, and the pooled
    planes are 37 x 62.  Forward with pool=True, the pooled data gradient, the pooled weight + bias gradient (from the forward's
    transformed activations).  (c) as test_conv3x3_f32_fused_relu_maxpool: the pooled values against float64 (2e-5); the gradients against
    float64 with the window selection decoded from the DEVICE words (dx 2e-5, dw / db 1e-4)."""
    Cin, Cout, H, W = 64, 128, 75, 125
    g0 = torch.Generator().manual_seed(H + Cin)
    x = torch.randn(1, Cin, H, W, generator=g0)
    wt = torch.randn(Cout, Cin, 3, 3, generator=g0) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g0) * 0.2
    Hp, Wp = H // 2, W // 2
    dp = torch.randn(1, Cout, Hp, Wp, generator=g0)

    def case(g):
        xd, wd, bd, dpd = (g.place(t.to(DEV)) for t in (x, wt, b, dp))
        (yp,), xt, bits = ops.conv3x3_fwd([xd], wd, bd, True, keep_transformed=True, want_bits=True, pool=True)
        g.outputs(x_transformed=xt)
        dx = ops.conv3x3_bwd_data([dpd], wd, bits, pooled_from=[(H, W)])[0]
        dw, db = ops.conv3x3_wgrad([xd], [dpd], bits, want_bias=True, x_transformed=xt, pooled=True)
        th, tw = (H + 3) // 4, (W + 3) // 4
        return {"y_pooled": yp, "dx": dx, "dw": dw, "db": db, "window_words": bits.view(Cout, -1)[:, :th * tw]}       # the defined words: one per (channel, 4 x 4 tile)
    out = both(case)
    pre = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    close(out["y_pooled"], F.max_pool2d(pre.clamp_min(0), 2, 2), 2e-5, scale_floor=max(1.0, float(pre.abs().max())))
    th, tw = (H + 3) // 4, (W + 3) // 4
    words = out["window_words"].cpu().to(torch.int32).bitwise_and(0xFFFF).view(Cout, th, tw)
    sel = torch.zeros(Cout, 4 * th, 4 * tw, dtype=torch.float64)
    for k in range(4):                                        # window k = wi * 2 + wj of a tile: bits 3k .. 3k + 1 = position of the maximum, bit 3k + 2 = maximum > 0
        w3 = (words >> (3 * k)) & 7
        for pos in range(4):
            sel[:, (k // 2) * 2 + pos // 2::4, (k % 2) * 2 + pos % 2::4] = (w3 == (4 | pos)).double()
    up = torch.zeros(1, Cout, H, W, dtype=torch.float64)
    up[:, :, :2 * Hp, :2 * Wp] = dp.double().repeat_interleave(2, 2).repeat_interleave(2, 3)
    gfull = up * sel[:, :H, :W]
    close(out["dx"], F.conv_transpose2d(gfull, wt.double(), None, padding=1), 2e-5)
    close(out["dw"], torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), gfull, padding=1), 1e-4)
    close(out["db"], gfull.sum(dim=(0, 2, 3)), 1e-4)


def test_gemm_nt(ops, products):
    """(64, 192, 96): one 64-row tile of A, three of B, K = 3 x 32.  (c) float64: 1e-5 * sqrt(K) * 4 absolute
    (test_gemm_nt_and_the_1x1_convolution_weight_gradient).  At this shape K is not split, so the result IS the kernel's buffer and is
    declared like any output (asserted: a split product would be a sum torch makes, and its buffer would need g.expect_arenas)."""
    M, Nn, K = 64, 192, 96
    g0 = torch.Generator().manual_seed(M + K)
    a, b = torch.randn(M, K, generator=g0), torch.randn(Nn, K, generator=g0)
    assert ops._gemm_nt_splits(M, Nn, K) == 1
    out = both(lambda g: {"out": ops.gemm_nt(g.place(a.to(DEV)), g.place(b.to(DEV)))})
    assert float((out["out"].double().cpu() - a.double() @ b.double().t()).abs().max()) < 1e-5 * K ** 0.5 * 4


# ============================================================================================ first convolution (csrc/conv_c3.hip)
@pytest.mark.parametrize("Cout,H,W", [(32, 9, 700), (80, 33, 257), (16, 1, 1)], ids=["wide", "two_words", "one_pixel"])
def test_conv3x3_c3(ops, Cout, H, W):
    """(c) float64, mask from the device output: forward 1e-5, weight and bias gradient 1e-4 of the scale (test_conv3x3_c3_first_convolution)."""
    g0 = torch.Generator().manual_seed(Cout + W)
    x = torch.randn(1, 3, H, W, generator=g0)
    wt = torch.randn(Cout, 3, 3, 3, generator=g0) * 0.3
    b = torch.randn(Cout, generator=g0) * 0.2
    dy = torch.randn(1, Cout, H, W, generator=g0)

    def case(g):
        xd, wd, bd, dyd = (g.place(t.to(DEV)) for t in (x, wt, b, dy))
        y, bits = ops.conv3x3_c3_fwd(xd, wd, bd, True, want_bits=True)
        dw, db = ops.conv3x3_c3_wgrad(xd, dyd, bits)
        dw0, _ = ops.conv3x3_c3_wgrad(xd, dyd, None)
        return {"y": y, "relu_bits": bits, "linear": ops.conv3x3_c3_fwd(xd, wd, None, False), "dw": dw, "db": db, "dw_no_relu": dw0}
    out = both(case)
    pre = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    scale = max(1.0, float(pre.abs().max()))
    assert float((out["y"].double().cpu() - pre.clamp_min(0)).abs().max()) < 1e-5 * scale
    assert float((out["linear"].double().cpu() - F.conv2d(x.double(), wt.double(), None, padding=1)).abs().max()) < 1e-5 * scale
    mask = out["y"].cpu() > 0
    got = (out["relu_bits"].cpu()[:, None] >> torch.arange(64)[None, :, None, None]) & 1      # bit co % 64 of word [co / 64][pixel] (include/frcnn_hip.h)
    assert torch.equal(got.reshape(-1, H, W)[:Cout].bool(), mask[0])
    gm = dy.double() * mask
    close(out["dw"], torch.nn.grad.conv2d_weight(x.double(), (Cout, 3, 3, 3), gm, padding=1), 1e-4)
    close(out["db"], gm.sum(dim=(0, 2, 3)), 1e-4)
    close(out["dw_no_relu"], torch.nn.grad.conv2d_weight(x.double(), (Cout, 3, 3, 3), dy.double(), padding=1), 1e-4)


# ============================================================================================ frozen norm (csrc/affine.hip)
AFFINE_HW = [(1, 1), (1, 1023), (32, 32), (25, 41), (37, 53)]               # HW = 1, 1023, 1024, 1025, 1961: around the 1024-element piece of a workgroup


def _affine_ref(x, scale, shift, r, relu):
    ref = x * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)
    if r is not None:
        ref = ref + r
    return torch.relu(ref) if relu else ref


@pytest.mark.parametrize("H,W", AFFINE_HW)
@pytest.mark.parametrize("with_res,relu", [(False, True), (True, True), (True, False)])
def test_affine_act(ops, H, W, with_res, relu):
    """C = 5.  (c) the torch expression relu(x * scale + shift + res) under autograd on the device: values and gradients bit for bit
    (test_affine_act_is_the_torch_form_bit_for_bit)."""
    g0 = torch.Generator().manual_seed(5 + with_res * 2 + relu)
    C_ = 5
    x = torch.randn(1, C_, H, W, generator=g0).to(DEV)
    r = torch.randn(1, C_, H, W, generator=g0).to(DEV) if with_res else None
    scale, shift = (torch.rand(C_, generator=g0) + 0.5).to(DEV), torch.randn(C_, generator=g0).to(DEV)
    dy = torch.randn(1, C_, H, W, generator=g0).to(DEV)

    def case(g):
        xs = [g.place(x.clone().requires_grad_(True))] + ([g.place(r.clone().requires_grad_(True))] if with_res else [])
        y = ops.affine_act(xs[0], g.place(scale), g.place(shift), xs[1] if with_res else None, relu)
        grads = torch.autograd.grad(y, xs, g.place(dy))
        return dict({"y": y}, **dict(zip(("dx", "dres"), grads)))
    # without a ReLU the residual's gradient is the incoming gradient itself (ops._AffineActFn.backward): the test's own placed tensor
    out = both(case)
    leaves = [x.clone().requires_grad_(True)] + ([r.clone().requires_grad_(True)] if with_res else [])
    ref = _affine_ref(leaves[0], scale, shift, leaves[1] if with_res else None, relu)
    want = torch.autograd.grad(ref, leaves, dy)
    assert torch.equal(out["y"], ref.detach())
    for k, w_ in zip(("dx", "dres"), want):
        assert torch.equal(out[k], w_), k


@pytest.mark.parametrize("H,W", AFFINE_HW)
@pytest.mark.parametrize("form", ["inner", "stream", "stream_res_twin", "f32_res_twin"])
def test_affine_act_mixed(ops, H, W, form):
    """The four mixed forms, C = 5.  (c) the autocast torch expressions, values, twin and gradients bit for bit
    (test_affine_act_mixed_is_the_autocast_torch_form)."""
    g0 = torch.Generator().manual_seed(11)
    C_ = 5
    with_res, twin, inner = form.endswith("res_twin"), form.endswith("twin"), form == "inner"
    x = torch.randn(1, C_, H, W, generator=g0).to(DEV)
    x = x.bfloat16() if form != "f32_res_twin" else x
    r = torch.randn(1, C_, H, W, generator=g0).to(DEV) if with_res else None
    scale, shift = (torch.rand(C_, generator=g0) + 0.5).to(DEV), torch.randn(C_, generator=g0).to(DEV)
    dy = torch.randn(1, C_, H, W, generator=g0).to(DEV)
    dy = dy.bfloat16() if inner else dy
    dt = torch.randn(1, C_, H, W, generator=g0).to(DEV).bfloat16() if twin else None

    def case(g):
        xs = [g.place(x.clone().requires_grad_(True))] + ([g.place(r.clone().requires_grad_(True))] if with_res else [])
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = ops.affine_act_mixed(xs[0], g.place(scale), g.place(shift), xs[1] if with_res else None, relu=True, out_bf16=inner, twin=twin)
        y, yt = out if twin else (out, None)
        grads = torch.autograd.grad([y] + ([yt] if twin else []), xs, [g.place(dy)] + ([g.place(dt)] if twin else []))
        return dict({"y": y, "twin": yt}, **dict(zip(("dx", "dres"), grads)))
    out = both(case)
    leaves = [x.clone().requires_grad_(True)] + ([r.clone().requires_grad_(True)] if with_res else [])
    ref32 = _affine_ref(leaves[0].float(), scale, shift, leaves[1] if with_res else None, True)
    ref, ref_twin = (ref32.bfloat16() if inner else ref32), (ref32.bfloat16() if twin else None)
    want = torch.autograd.grad([ref] + ([ref_twin] if twin else []), leaves, [dy] + ([dt] if twin else []))
    assert out["y"].dtype == ref.dtype and torch.equal(out["y"], ref.detach())
    if twin:
        assert torch.equal(out["twin"], ref_twin.detach())
    for k, w_ in zip(("dx", "dres"), want):
        assert out[k].dtype == w_.dtype and torch.equal(out[k], w_), k


def _same_with_nan(a, b):
    """bit for bit where neither is a NaN, NaN in the same places (a NaN's payload is not part of torch's contract)"""
    return a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a.float(), nan=7.0), torch.nan_to_num(b.float(), nan=7.0))


@pytest.mark.parametrize("form", ["f32", "f32_res", "inner", "stream", "stream_res_twin", "f32_res_twin"])
def test_affine_act_relu_backward_passes_the_gradient_at_a_nan_output_like_torch(ops, form):
    """torch's ReLU backward (threshold_backward) is `y <= 0 ? 0 : g`: at a NaN output the gradient PASSES (on the CPU relu(nan).backward(5.)
    gives 5; this case asserts the same of the device, by comparing with the torch expression under autograd there).  The kernels computed
    `y > 0 ? g : 0` and dropped it.  A NaN and a -inf in x (test_affine_act_is_the_torch_form_bit_for_bit's poison): outputs and gradients
    equal to the torch form bit for bit, NaN positions included -- the fp32 op and the four mixed forms."""
    g0 = torch.Generator().manual_seed(17)
    C_, H, W = 5, 25, 41
    mixed = not form.startswith("f32") or form == "f32_res_twin"
    with_res, twin, inner = form.endswith(("res", "res_twin")), form.endswith("twin"), form == "inner"
    x = torch.randn(1, C_, H, W, generator=g0).to(DEV)
    x[0, 3, 5, 7] = float("nan")
    x[0, 4, 0, 0] = float("-inf")
    x[0, 1, 24, 40] = float("nan")                            # in the tail of the last piece
    x = x.bfloat16() if mixed and form != "f32_res_twin" else x
    r = torch.randn(1, C_, H, W, generator=g0).to(DEV) if with_res else None
    scale, shift = (torch.rand(C_, generator=g0) + 0.5).to(DEV), torch.randn(C_, generator=g0).to(DEV)
    dy = torch.randn(1, C_, H, W, generator=g0).to(DEV)
    dy = dy.bfloat16() if inner else dy
    dt = torch.randn(1, C_, H, W, generator=g0).to(DEV).bfloat16() if twin else None
    leaves = [x.clone().requires_grad_(True)] + ([r.clone().requires_grad_(True)] if with_res else [])
    ref32 = _affine_ref(leaves[0].float() if mixed else leaves[0], scale, shift, leaves[1] if with_res else None, True)
    ref, ref_twin = (ref32.bfloat16() if inner else ref32), (ref32.bfloat16() if twin else None)
    want = torch.autograd.grad([ref] + ([ref_twin] if twin else []), leaves, [dy] + ([dt] if twin else []))
    assert bool(torch.isnan(ref[0, 3, 5, 7])) and float(ref.detach()[0, 4, 0, 0]) == 0.0
    assert float(want[0][0, 3, 5, 7].float()) != 0.0 and float(want[0][0, 4, 0, 0].float()) == 0.0        # the premise: torch passes the gradient at the NaN, drops it at -inf
    xs = [x.clone().requires_grad_(True)] + ([r.clone().requires_grad_(True)] if with_res else [])
    if mixed:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = ops.affine_act_mixed(xs[0], scale, shift, xs[1] if with_res else None, relu=True, out_bf16=inner, twin=twin)
    else:
        out = ops.affine_act(xs[0], scale, shift, xs[1] if with_res else None, True)
    y, yt = out if twin else (out, None)
    got = torch.autograd.grad([y] + ([yt] if twin else []), xs, [dy] + ([dt] if twin else []))
    assert _same_with_nan(y.detach(), ref.detach()) and (not twin or _same_with_nan(yt.detach(), ref_twin.detach()))
    for a_, w_ in zip(got, want):
        assert _same_with_nan(a_, w_)
    assert float(got[0][0, 3, 5, 7].float()) == float(want[0][0, 3, 5, 7].float())


# ============================================================================================ loss, detection
import test_gpu_loss as tl                                    # noqa: E402  (exact_case / ref64 / the derived bounds of that file)


def test_detection_loss(ops):
    """The smallest EXACT_SHAPES of test_gpu_loss.py, (N, R, NC) = (300, 5, 64), through ops.detection_loss and autograd of the total.
    The four gradients that autograd returns are torch's products of the kernel's un-normalised gradients with a scalar (derived); the
    kernel's own buffers -- out [7] and the four gradients, allocated in _DetLossFn.forward -- are asserted to be arenas by g.expect_arenas
    (the five losses are views of out and declared as usual).  (c) as test_gpu_loss.py: the five losses one fp32
    bit pattern (exact data); SmoothL1' gradients bit for bit (the kernel's rows in numpy float32 times fl(1 / n)); class gradients
    within class_grad_bound of float64."""
    Nn, R, NC = tl.EXACT_SHAPES[-1]
    c, e = tl.exact_case(Nn, R, NC, tl.rpn_seams(Nn)[0])

    def case(g):
        leaves = [g.place(T(c[k]).requires_grad_(True)) for k in tl.PRED]
        out = ops.detection_loss([leaves[0].unsqueeze(0), leaves[1].unsqueeze(0), leaves[2], leaves[3]], [g.place(T(c[k])) for k in tl.TGT])
        g.expect_arenas("forward", [(7,), (Nn, 2), (Nn, 4), (R, NC), (R, 4)])
        grads = torch.autograd.grad(out[0], leaves)
        return dict({"loss%d" % i: o.detach() for i, o in enumerate(out)}, **{"d_" + k: t for k, t in zip(tl.PRED, grads)})
    out = both(case, derived=tuple("d_" + k for k in tl.PRED))
    losses = np.array([float(out["loss%d" % i]) for i in range(5)], np.float32)
    assert losses.tobytes() == e["losses"].tobytes(), (losses, e["losses"])
    nv = float((c["trc"] >= 0).sum())
    r = tl.ref64(c)
    s_rpn, s_head = np.float32(1) / np.float32(nv), np.float32(1) / np.float32(R)
    assert np.array_equal(N(out["d_rr"]), tl.sl1_f32(c["rr"], c["trr"], c["trc"] > 0, tl.BETA_RPN)[1] * s_rpn)
    assert np.array_equal(N(out["d_hr"]), tl.sl1_f32(c["hr"], c["tr"], c["tc"] > 0, tl.BETA_HEAD)[1] * s_head)
    assert np.abs(N(out["d_rc"]).astype(np.float64) * nv - r["g"][0]).max() <= tl.class_grad_bound(2)
    assert np.abs(N(out["d_hc"]).astype(np.float64) * R - r["g"][2]).max() <= tl.class_grad_bound(NC)


import test_gpu_detect as td                                  # noqa: E402
from oracle import model_ref                                  # noqa: E402


@pytest.mark.parametrize("P,C_,n,thr,seed", [(7, 3, 7, 0.05, 3), (1, 3, 1, 0.05, 6), (300, 21, 173, 0.05, 4)], ids=["7x3", "1x3", "300x21_173_live"])
def test_detect_postprocess(ops, P, C_, n, thr, seed):
    """Defined part: the first count[0] rows of boxes / labels / scores, count, class_counts, and the first n_rois rows of prob (rows at and
    above the device count n_rois are ignored: the head ran on padding there).  (c) oracle/model_ref.ref_predict_post: labels bit for bit,
    scores and boxes bit for bit with NaN in the same places; the softmax within 1e-6 of torch's (test_gpu_detect._check_vs_oracle)."""
    hc, hr, rois = td._inputs(P, C_, seed, n=n)

    def case(g):
        det = ops.detect_postprocess(g.place(T(hc)), g.place(T(hr)), g.place(T(rois)), g.place(T(np.array([n], np.int32))), thr, 0.3, want_prob=True)
        m = int(det.count.item())
        return {"count": det.count, "class_counts": det.class_counts, "boxes": det.boxes[:m], "labels": det.labels[:m], "scores": det.scores[:m], "prob": det.prob[:n]}
    out = both(case)
    prob = N(out["prob"])
    rb, rl, rs, _, _ = model_ref.ref_predict_post(hc[:n], hr[:n], rois[:n], C_, thr, prob=prob)
    assert int(out["count"].item()) == len(rl) and np.array_equal(N(out["class_counts"]), np.bincount(rl, minlength=C_ - 1))
    assert np.array_equal(N(out["labels"]), rl) and td._same_bits(N(out["scores"]), rs) and td._same_bits(N(out["boxes"]), rb)
    live = np.isfinite(hc[:n]).all(1)
    cpu_sm = torch.softmax(torch.from_numpy(hc[:n]), dim=-1).numpy()
    assert np.abs(prob[live] - cpu_sm[live]).max(initial=0) < 1e-6 and np.array_equal(np.isnan(prob), np.isnan(cpu_sm))


# ============================================================================================ evaluators
import coco_eval_ref                                          # noqa: E402
import eval_merge_ref                                         # noqa: E402
import eval_ref                                               # noqa: E402
import test_gpu_coco_eval as tc                               # noqa: E402
import test_gpu_eval as te                                    # noqa: E402
import test_gpu_eval_merge as tm                              # noqa: E402


def _store(g, prefix, ev, kind):
    """The defined part of an evaluator's buffers: the record columns up to the cursor, the ledger up to its count, the counters.
    VOC reserves a frame's slots with ONE atomic add, so slot order is defined.  The COCO update runs one workgroup per category and each
    reserves its slots with its own atomic add on the cursor (csrc/coco_eval.hip): inside a frame's slot range the categories land in
    arrival order, so the store is defined as a SET of rows -- the raw columns are declared (arena, guards) and compared after sorting
    the rows by (image_id, label, rank), which is unique per record."""
    n = min(int(ev.cursor.item()), ev.record_capacity)
    cols = {prefix + k: t[:n] for k, t in zip(ev._keys(), ev._records())}
    if kind == "coco":
        g.outputs(**{k.replace(".", "_raw_"): t for k, t in cols.items()})
        key = np.lexsort((N(ev._rec_order[:n]), N(ev.rec_label[:n]), N(ev.rec_image[:n])))
        assert n == 0 or len(set(zip(N(ev.rec_image[:n]).tolist(), N(ev.rec_label[:n]).tolist(), N(ev._rec_order[:n]).tolist()))) == n
        cols = {k + ".sorted": t[torch.from_numpy(key).to(t.device)] for k, t in cols.items()}
    d = dict(cols)
    d.update({prefix + "counter": ev._counter, prefix + "cursor": ev.cursor, prefix + "error": ev.error})
    if ev.image_capacity:
        m = min(int(ev.led_count.item()), ev.image_capacity)
        d.update({prefix + "led_image": ev.led_image[:m], prefix + "led_range": ev.led_range[:m], prefix + "led_delta": ev.led_delta[:m],
                  prefix + "led_count": ev.led_count, prefix + "snap_cursor": ev._snap_cursor, prefix + "snap_counter": ev._snap_counter})
    return d


@pytest.mark.parametrize("kind", tm.KINDS)
def test_evaluators_update_ledger_merge_and_summary(ops, kind):
    """Six frames of test_gpu_eval_merge's pool (at most 64 detections, 16 ground truths, 6 classes): `one` evaluator sees all six (update,
    ledger append, AP / accumulate); shards A (frames 0-3) and B (frames 2-5) are merged on the device into a poisoned third.  Evaluators,
    their ground-truth buffers and workspaces are built inside the guarded context, so every buffer is an arena; the detections are placed.
    The record stores are compared up to the cursor, the ledgers up to their count.
    (c) VOC: records = tests/eval_ref.py bit for bit, AP within npos * 2^-52 (test_gpu_eval._check_set); COCO: records, precision, recall,
    npig and stats = tests/coco_eval_ref.py bit for bit (test_gpu_coco_eval._check); the merge = tests/eval_merge_ref.py bit for bit."""
    frames = tm._pool(kind)[:6]

    def feed(g, fd, f):
        if kind == "voc":
            fd.gt.set(f["gt_boxes"], f["gt_labels"], f["gt_difficult"], (f["w"], f["h"]), f["image_id"])
        else:
            fd.gt.set(f["gt_boxes"], f["gt_labels"], f["gt_iscrowd"], f["gt_area"], orig_wh=(f["w"], f["h"]), image_id=f["image_id"])
        d = tm._dets(f)
        fd.ev.update(ops.Detections(*[None if t is None else g.place(t) for t in d]), fd.gt)

    def case(g):
        one, a, b = (tm._Feeder(kind, tm._ev(kind, record_capacity=1 << 10, image_capacity=32)) for _ in range(3))
        for k, f in enumerate(frames):
            feed(g, one, f)
            if k < 4:
                feed(g, a, f)
            if k >= 2:
                feed(g, b, f)
        merged = tm._ev(kind, record_capacity=1 << 10, image_capacity=32)
        tm._poison(merged)
        hosts = [tm._host(a.ev), tm._host(b.ev)]
        merged.merge_shards([a.ev, b.ev.state()])
        out = dict(_store(g, "one.", one.ev, kind), **_store(g, "merged.", merged, kind))
        res = one.ev.summarize()
        out.update({"summary." + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in res.items() if isinstance(v, np.ndarray)})
        out.update(_records=one.ev.records_sorted(), _res=res, _merged=tm._host(merged), _merged_res=merged.summarize(), _hosts=hosts)
        return out
    out = both(case, derived=lambda k: k.endswith(".sorted"))
    if kind == "voc":
        rec, npos = eval_ref.sequential(frames, tm.NC, tm.THR)
        te._same_records(out["_records"], rec)
        assert np.array_equal(out["_res"]["npos"], npos) and out["_res"]["n_records"] == len(rec["label"])
        te._ap_within_bound(out["_res"]["ap"], eval_ref.average_precision(rec, npos, len(tm.THR))[0], npos)
    else:
        r = coco_eval_ref.run(frames, tm.NC)
        tc._same_records(out["_records"], r["records"])
        tc._same_result(out["_res"], r)
    eval_merge_ref.same(out["_merged"], eval_merge_ref.merge(out["_hosts"], 1 << 10, 32), kind)
    tm._same_summary(kind, out["_merged_res"], out["_res"])                               # six distinct images either way


# ============================================================================================ input stage
import crop_ref                                               # noqa: E402
import mosaic_ref                                             # noqa: E402
import photometric_ref                                        # noqa: E402


def _u8(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# W = 7 and W = 21: 3 * W = 21 and 63 bytes per row, no multiple of 4 or of 16 -- every uint8 row ends inside a vector
ODD_FRAMES = [(5, 7), (9, 21)]


@pytest.mark.parametrize("name", ["up", "down_flip", "same_w"])
def test_preprocess_golden(TF, name):
    """(c) the Pillow / torch golden of tests/golden/preprocess.npz, bit for bit (test_hip_matches_pillow_golden)."""
    pre = np.load(__file__.rsplit("/", 1)[0] + "/golden/preprocess.npz")
    h, w, oh, ow, flip = (int(v) for v in pre[name + "_meta"])

    def case(g):
        f, u8 = TF.preprocess_image(g.place(T(pre[name + "_img"])), (oh, ow), None, bool(flip), want_u8=True)
        return {"f32": f, "u8": u8, "boxes": TF.preprocess_boxes(g.place(T(pre[name + "_boxes"])), (w, h), (ow, oh), bool(flip))}
    out = both(case)
    assert np.array_equal(N(out["u8"]), pre[name + "_u8"]) and np.array_equal(N(out["f32"]), pre[name + "_f32"])
    assert np.array_equal(N(out["boxes"]), pre[name + "_boxes_out"])


@pytest.mark.parametrize("hw,out_hw,pad_hw,flip", [((5, 7), (11, 21), (32, 32), False), ((9, 21), (4, 7), None, True), ((9, 21), (9, 21), (32, 32), False),
                                                   ((5, 7), (5, 3), (6, 5), True)])
def test_preprocess_rows_that_end_inside_a_vector(TF, hw, out_hw, pad_hw, flip):
    """Source and / or resized rows of 21 and 63 bytes, up- and down-scaling, a zero pad to the right and below.  (c) the oracle's
    restatement of Pillow's resampler + ToTensor / Normalize, bit for bit (test_hip_full_size_matches_pillow_digest_and_oracle)."""
    img = _u8(hw[0] * 31 + hw[1], *hw)
    rng = np.random.RandomState(3)
    boxes = (rng.rand(5, 4) * np.array([hw[1], hw[0], hw[1], hw[0]])).astype(np.float32)

    def case(g):
        f, u8 = TF.preprocess_image(g.place(T(img)), out_hw, pad_hw, flip, want_u8=True)
        return {"f32": f, "u8": u8, "boxes": TF.preprocess_boxes(g.place(T(boxes)), (hw[1], hw[0]), (out_hw[1], out_hw[0]), flip)}
    out = both(case)
    u8_o, f_o = orc.preprocess_image(img, out_hw, pad_hw, flip)
    assert np.array_equal(N(out["u8"]), u8_o) and np.array_equal(N(out["f32"]), f_o)
    assert np.array_equal(N(out["boxes"]), orc.preprocess_boxes(boxes, (hw[1], hw[0]), (out_hw[1], out_hw[0]), flip))


def _mosaic_case(TF, inp):
    imgs, boxes, labels, regions, size, max_size = inp
    counts = [len(b) for b in boxes]
    cat_b = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in boxes])
    cat_l = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l in labels])

    def case(g):                                              # tile-major boxes + counts: the form in which the op reads the test's own (placed) tensors
        res = TF.mosaic([g.place(T(im)) for im in imgs], g.place(T(cat_b)), g.place(T(cat_l)), regions, size, max_size, counts=counts)
        return {"canvas": res.canvas_u8, "boxes": res.boxes, "labels": res.labels, "count": res.count, "fallback": res.fallback}
    return both(case)


def _mosaic_check(out, ref):
    """(c) canvas, boxes, labels, fallback and count bit for bit; rows at and above the count are zeros (test_gpu_mosaic.check)"""
    canvas, boxes, labels, fallback = ref[:4]
    n = len(boxes)
    assert int(out["count"].item()) == n and np.array_equal(N(out["fallback"]), fallback) and np.array_equal(N(out["canvas"]), canvas)
    assert np.array_equal(N(out["boxes"])[:n], boxes) and np.array_equal(N(out["labels"])[:n], labels)
    assert not N(out["boxes"])[n:].any() and not N(out["labels"])[n:].any()


@pytest.mark.parametrize("name", mosaic_ref.SMALL)
def test_mosaic_golden(TF, name):
    """(c) the reference's own results (tests/golden/mosaic.npz) and the restatement tests/mosaic_ref.py."""
    gold = mosaic_ref.load_golden()
    inp = mosaic_ref.small_inputs(gold, name)
    out = _mosaic_case(TF, inp)
    _mosaic_check(out, (gold[name + "_canvas"], gold[name + "_boxes_out"], gold[name + "_labels_out"], gold[name + "_fallback"]))
    _mosaic_check(out, mosaic_ref.mosaic_ref(*inp))


def test_mosaic_rows_that_end_inside_a_vector(TF):
    """Four sources of width 7, 21, 7 and 21 (rows of 21 / 63 bytes), size 13: a 26 x 26 canvas whose rows are 78 bytes.  (c) tests/mosaic_ref.py."""
    size, max_size = 13, 1333
    hws = [(9, 7), (11, 21), (7, 7), (21, 21)]
    imgs = [_u8(70 + k, h, w) for k, (h, w) in enumerate(hws)]
    rng = np.random.RandomState(9)
    regions, boxes, labels = [], [], []
    for k, (h, w) in enumerate(hws):
        H1, W1 = mosaic_ref.first_resize_hw(h, w, size, max_size)
        regions.append([1, 1, max(H1 - 2, 1), max(W1 - 2, 1)])
        x1, y1 = rng.uniform(0, w * 0.5, 3), rng.uniform(0, h * 0.5, 3)
        boxes.append(np.stack([x1, y1, x1 + rng.uniform(1, w * 0.5, 3), y1 + rng.uniform(1, h * 0.5, 3)], 1).astype(np.float32))
        labels.append(np.arange(3 * k, 3 * k + 3, dtype=np.int64))
    inp = (imgs, boxes, labels, np.array(regions, np.int32), size, max_size)
    _mosaic_check(_mosaic_case(TF, inp), mosaic_ref.mosaic_ref(*inp))


def _small_golden(gold, names, key):
    """the name whose input frame has the fewest bytes"""
    return min(names, key=key)


def test_photometric_and_zoom_out_golden(TF):
    """The smallest golden case of each (tests/golden/photometric.npz: the reference's own code under Pillow), bit for bit
    (test_every_photometric_golden_case_..., test_every_zoom_out_golden_case_...)."""
    gold = photometric_ref.load_golden()
    pname = min(gold["p_names"].tolist(), key=lambda n: photometric_ref.case_input(gold, n).size)
    zname = min(gold["z_names"].tolist(), key=lambda n: gold[n + "_img"].size)
    pimg = photometric_ref.case_input(gold, pname)
    plan = TF.photometric_plan(gold[pname + "_order"].tolist(), gold[pname + "_factors"])

    def case(g):
        canvas, bo = TF.zoom_out(g.place(T(gold[zname + "_img"])), g.place(T(gold[zname + "_boxes"])), gold[zname + "_new_hw"], gold[zname + "_top_left"])
        return {"photometric": TF.photometric_distort(g.place(T(pimg)), g.place(T(np.asarray(plan, np.int32)))), "canvas": canvas, "boxes": bo}
    out = both(case)
    assert np.array_equal(N(out["photometric"]), photometric_ref.photometric(pimg, gold[pname + "_order"], gold[pname + "_factors"]))
    if pname + "_out" in gold.files:
        assert np.array_equal(N(out["photometric"]), gold[pname + "_out"])
    assert np.array_equal(N(out["canvas"]), gold[zname + "_canvas"]) and np.array_equal(N(out["boxes"]), gold[zname + "_boxes_out"])


@pytest.mark.parametrize("hw", ODD_FRAMES)
@pytest.mark.parametrize("order,factors", [((0, 1, 2, 3), (1.3, 0.7, 1.4, 0.05)), ((3, 2, 1, 0), (0.6, 1.5, 0.5, -0.08))])
def test_photometric_and_zoom_out_rows_that_end_inside_a_vector(TF, hw, order, factors):
    """(c) tests/photometric_ref.py (pinned to Pillow by tests/test_photometric_host.py), bit for bit."""
    img = _u8(hw[0] + hw[1], *hw)
    plan = TF.photometric_plan(list(order), np.asarray(factors, np.float64))
    rng = np.random.RandomState(4)
    boxes = (rng.rand(3, 4) * np.array([hw[1], hw[0], hw[1], hw[0]])).astype(np.float32)
    new_hw, top_left = (hw[0] * 2 + 1, hw[1] * 2 + 1), (3, 5)                 # canvas rows of 45 / 129 bytes, the frame pasted at an odd byte offset

    def case(g):
        canvas, bo = TF.zoom_out(g.place(T(img)), g.place(T(boxes)), new_hw, top_left)
        return {"photometric": TF.photometric_distort(g.place(T(img)), g.place(T(np.asarray(plan, np.int32)))), "canvas": canvas, "boxes": bo}
    out = both(case)
    assert np.array_equal(N(out["photometric"]), photometric_ref.apply_plan(img, np.asarray(plan, np.int32)))
    canvas_o, boxes_o = photometric_ref.zoom_out(img, boxes, new_hw, top_left)
    assert np.array_equal(N(out["canvas"]), canvas_o) and np.array_equal(N(out["boxes"]), boxes_o)


def _crop_case(TF, img, boxes, labels, crowd, resize_hw, region):
    def case(g):
        res = TF.crop(g.place(T(img)), g.place(T(np.asarray(boxes, np.float32).reshape(-1, 4))), g.place(T(labels)), region, resize_hw,
                      iscrowd=None if crowd is None else g.place(T(crowd)))
        return dict(zip(("img", "boxes", "labels", "area", "iscrowd", "count"), res))
    return both(case)


def _crop_check(out, ref):
    """(c) image, boxes, labels, area, iscrowd and count bit for bit; rows at and above the count are zeros (test_gpu_crop.check)"""
    img, boxes, labels, area, crowd = ref
    n = len(boxes)
    assert int(out["count"].item()) == n and np.array_equal(N(out["img"]), img)
    assert np.array_equal(N(out["boxes"])[:n], boxes) and np.array_equal(N(out["labels"])[:n], labels) and np.array_equal(N(out["area"])[:n], area)
    for k in ("boxes", "labels", "area"):
        assert not N(out[k])[n:].any()
    if crowd is not None:
        assert np.array_equal(N(out["iscrowd"])[:n], crowd) and not N(out["iscrowd"])[n:].any()


def test_crop_golden(TF):
    """The two smallest golden cases of tests/golden/crop.npz, a plain crop and a resize + crop where the file has both.  (c) the
    reference's own results and tests/crop_ref.py."""
    gold = crop_ref.load_golden()
    names = sorted(crop_ref.case_names(gold), key=lambda n: crop_ref.case_inputs(gold, n)[0].size)
    picked = names[:1] + [n for n in names[1:] if int(gold[n + "_meta"][8]) != int(gold[names[0] + "_meta"][8])][:1]
    for name in picked:
        inp = crop_ref.case_inputs(gold, name)
        plain = not int(gold[name + "_meta"][8])
        out = _crop_case(TF, inp[0], inp[1], inp[2], inp[3], None if plain else inp[4], inp[5])
        _crop_check(out, (gold[name + "_img_out"], gold[name + "_boxes_out"], gold[name + "_labels_out"], gold[name + "_area_out"],
                          gold[name + "_iscrowd_out"] if inp[3] is not None else None))
        _crop_check(out, crop_ref.crop_ref(*inp))


@pytest.mark.parametrize("hw,hw1,region,n", [((5, 7), (5, 7), (1, 2, 3, 5), 4), ((9, 21), (13, 29), (2, 4, 9, 21), 6), ((9, 21), (5, 7), (0, 0, 5, 7), 3),
                                             ((5, 7), (15, 21), (3, 0, 10, 21), 65)])
def test_crop_rows_that_end_inside_a_vector(TF, hw, hw1, region, n):
    """Source, resized and cropped rows of 21 / 63 / 15 bytes; a plain crop, up- and down-scaling; 65 boxes = one past a wave.
    (c) tests/crop_ref.py, bit for bit (test_seeded_frames_equal_restatement_...)."""
    img, boxes, labels, crowd = crop_ref.seeded_case(50 + n, hw[0], hw[1], hw1, region, n)
    out = _crop_case(TF, img, boxes, labels, crowd, None if hw1 == hw else hw1, region)
    _crop_check(out, crop_ref.crop_ref(img, boxes, labels, crowd, hw1, region))
