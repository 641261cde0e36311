"""The number of ground-truth boxes as device data (frcnn_rpn_targets_n / frcnn_head_targets_n; ops.rpn_targets(n_gt=) /
ops.head_targets(n_gt=, empty=)).

The yardstick is the classic entry point on gt[:G].contiguous(): outputs, counts and the Philox state must be the same BITS.  The
rows at and above n_gt are adverse in three ways, in separate cases: all NaN; +-inf / 1e30; exact copies of anchors (RPN) or of RoIs
(head), which would win every match if a kernel read them.  After every call the zero-kept part of the RPN maker's control workspace is
zero.  What the reference does not define (it raises): n_gt <= 0 and n_gt > capacity -- docs/PARITY.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, OFFSET = 4242, 17
G_CAP = 130
PADS = ("nan", "inf", "copies")
# csrc/targets.hip carve_rpn: RpnCtl (1280 bytes: counts at 0, the Philox snapshot at 16 -- not cleared --, flag / arrival / ticket lines from 64 on), the
# staged form's snapshot (256), one 64-byte line per GT box for RPN_MAX_G = 4096 boxes, then the sampler's histogram and list counters (RpnSel2)
WS_ZERO = ((0, 16), (64, 1280), (1536, 1536 + 4096 * 64 + 2 * 2048 * 4 + 8))


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def rand_boxes(rng, n, lo=0.05, hi=0.5):
    c = rng.rand(n, 2) * 0.7 + 0.15
    wh = rng.rand(n, 2) * (hi - lo) + lo
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


_DATA = {}


def rpn_data(N):
    """gt [G_CAP, 4] and N anchors: a fifth of them jittered copies of gt boxes (IoU >= 0.7: more than 128 positives from a few boxes on),
    the rest random, so both classes are sampled.  Shared by the cases; never modified."""
    if N not in _DATA:
        rng = np.random.RandomState(N % 9973)
        gt = rand_boxes(rng, G_CAP, 0.1, 0.5)
        a = rand_boxes(rng, N, 0.03, 0.6)
        k = np.arange(0, N, 5)
        a[k] = np.clip(gt[rng.randint(0, G_CAP, k.size)] + (rng.rand(k.size, 4).astype(np.float32) - 0.5) * 0.01, 0, 1)
        _DATA[N] = (T(a), T(gt))
    return _DATA[N]


def padded(gt, n_live, pad, copies_of):
    """gt with the rows >= n_live replaced by the adverse padding"""
    out = gt.clone()
    m = out.shape[0] - n_live
    if m <= 0:
        return out
    if pad == "nan":
        out[n_live:] = float("nan")
    elif pad == "inf":
        v = torch.tensor([[-float("inf"), -1e30, float("inf"), 1e30], [1e30, float("inf"), -1e30, -float("inf")]], device=gt.device)
        out[n_live:] = v.repeat((m + 1) // 2, 1)[:m]
    else:
        out[n_live:] = copies_of[torch.arange(m, device=gt.device) % copies_of.shape[0]]
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and G.first_difference(a, b) is None


def ws_is_zero(ops):
    ws = ops._CTRL[("rpn_targets", torch.device(DEV).index)]
    return all(not bool(ws[lo:hi].any()) for lo, hi in WS_ZERO)


def staged_n():
    return 2 * torch.cuda.get_device_properties(DEV).multi_processor_count * 1024 + 1


# ------------------------------------------------------------------------------------------------ RPN maker
# 2 000 / 24 576: one launch (sampling inline) and its upper edge; 24 577: + rpn_apply_kernel; "staged": the grid no longer fits the chip
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("n_anchors", [2000, 24576, 24577, "staged"])
@pytest.mark.parametrize("variant", [0, 1])
def test_rpn_device_count_equals_the_sliced_call(ops, variant, n_anchors, pad):
    N = staged_n() if n_anchors == "staged" else n_anchors
    a, gt = rpn_data(N)
    sampled = 0
    for n_gt in (1, 63, 64, 65, 130):                                         # the seams of phase 1's 64-wide rounds
        st_ref, st_got = ops.philox_state(SEED, OFFSET, DEV), ops.philox_state(SEED, OFFSET, DEV)
        ref = ops.rpn_targets(a, gt[:n_gt].contiguous(), variant=variant, philox_state=st_ref)
        assert ws_is_zero(ops)
        got = ops.rpn_targets(a, padded(gt, n_gt, pad, a), variant=variant, philox_state=st_got, n_gt=i32(n_gt))
        what = (variant, N, pad, n_gt)
        for r, g_ in zip(ref, got):
            assert same_bits(r, g_), what
        assert torch.equal(st_ref, st_got) and st_got.cpu().tolist()[1] == OFFSET + 1, what
        assert ws_is_zero(ops), what
        c = got[2].cpu().tolist()
        assert c[2] == 0 and c[3] == 0, what
        sampled += c[0] > 128 and c[1] > 256
    assert sampled >= 3                                                        # the sampler did run for both classes (a property of the data)
    # (seed, offset) by value take the same path
    ref = ops.rpn_targets(a, gt[:65].contiguous(), variant=variant, seed=SEED, offset=OFFSET)
    got = ops.rpn_targets(a, padded(gt, 65, pad, a), variant=variant, seed=SEED, offset=OFFSET, n_gt=i32(65))
    assert all(same_bits(r, g_) for r, g_ in zip(ref, got)) and ws_is_zero(ops)


@pytest.mark.parametrize("variant", [0, 1])
def test_rpn_device_count_in_parity_mode(ops, variant):
    """perm_pos / perm_neg learned from a first call's counts, as the models' host mode does."""
    a, gt = rpn_data(2000)
    n_gt = 65
    gp = padded(gt, n_gt, "copies", a)
    n_pos, n_neg = ops.rpn_targets(a, gp, variant=variant, n_gt=i32(n_gt))[2].cpu().tolist()[:2]
    assert [n_pos, n_neg] == ops.rpn_targets(a, gt[:n_gt].contiguous(), variant=variant)[2].cpu().tolist()[:2]
    assert n_pos > 128 and n_neg > 256 - 128                                   # both permutations are consumed
    g = torch.Generator().manual_seed(3)
    pp, pn = torch.randperm(n_pos, generator=g), torch.randperm(n_neg, generator=g)
    ref = ops.rpn_targets(a, gt[:n_gt].contiguous(), variant=variant, perm_pos=pp, perm_neg=pn)
    got = ops.rpn_targets(a, gp, variant=variant, perm_pos=pp, perm_neg=pn, n_gt=i32(n_gt))
    assert all(same_bits(r, g_) for r, g_ in zip(ref, got))
    assert got[2].cpu().tolist()[2] == 0 and int((got[0] == 1).sum()) == 128 and int((got[0] == 0).sum()) == 128
    assert ws_is_zero(ops)
    # a wrong permutation length is still reported, next to the count's own bit
    bad = ops.rpn_targets(a, padded(gt, G_CAP, "nan", a), variant=variant, perm_pos=pp[:-1], perm_neg=pn, n_gt=i32(G_CAP + 1))[2].cpu().tolist()
    assert bad[2] & 16 and bad[2] & 3


# ------------------------------------------------------------------------------------------------ head maker
HEAD_CONFIGS = {0: dict(variant=0, label_offset=1, max_pos=32, total=128), 1: dict(variant=1, label_offset=0, max_pos=128, total=512)}
P_CAP, HG_CAP = 300, 20


def head_data():
    if "head" not in _DATA:
        rng = np.random.RandomState(77)
        gt = rand_boxes(rng, HG_CAP, 0.1, 0.5)
        rois = rand_boxes(rng, P_CAP, 0.03, 0.6)
        k = np.arange(0, P_CAP, 3)
        rois[k] = np.clip(gt[rng.randint(0, HG_CAP, k.size)] + (rng.rand(k.size, 4).astype(np.float32) - 0.5) * 0.02, 0, 1)
        lab = rng.randint(1, 20, HG_CAP).astype(np.int64)
        _DATA["head"] = (T(rois), T(gt), T(lab))
    return _DATA["head"]


def padded_labels(lab, n_live):
    out = lab.clone()
    out[n_live:] = 1 << 40                                                     # would show in a class if it were read
    return out


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("config", [0, 1])
def test_head_device_count_equals_the_sliced_call(ops, config, pad):
    rois, gt, lab = head_data()
    kw = HEAD_CONFIGS[config]
    for n_rois in (0, 1, 300):
        for n_gt in (1, 2, HG_CAP):
            what = (config, pad, n_rois, n_gt)
            st_ref, st_got = ops.philox_state(SEED, OFFSET, DEV), ops.philox_state(SEED, OFFSET, DEV)
            empty = i32(7)
            ref = ops.head_targets(rois, gt[:n_gt].contiguous(), lab[:n_gt].contiguous(), n_rois=i32(n_rois), want_keep=True, philox_state=st_ref, **kw)
            got = ops.head_targets(rois, padded(gt, n_gt, pad, rois), padded_labels(lab, n_gt), n_rois=i32(n_rois), want_keep=True, philox_state=st_got,
                                   n_gt=i32(n_gt), empty=empty, **kw)
            for r, g_ in zip(ref, got):                                        # cls, reg, sample_rois, keep index, counts
                assert same_bits(r, g_), what
            assert torch.equal(st_ref, st_got) and st_got.cpu().tolist()[1] == OFFSET + 1, what
            assert empty.item() == 0, what
            if n_rois == 300 and kw["total"] <= 300:                            # (total = 512 cannot be filled from 300 + n_gt candidates)
                assert got[4].cpu().tolist()[2:] == [kw["total"], 0], what       # every row sampled: the comparison is not one of empty results


# ------------------------------------------------------------------------------------------------ what the reference does not define
@pytest.mark.parametrize("n_gt", [0, -3])
@pytest.mark.parametrize("variant", [0, 1])
def test_no_live_box_marks_everything_and_the_next_frame_is_served(ops, L, variant, n_gt):
    a, gt = rpn_data(24577 if variant else 2000)
    rois, hgt, lab = head_data()
    kw = HEAD_CONFIGS[variant]
    st = ops.philox_state(SEED, OFFSET, DEV)
    status, empty = i32(0), i32(0)
    cls, reg, counts = ops.rpn_targets(a, padded(gt, 0, "copies", a), variant=variant, philox_state=st, n_gt=i32(n_gt))
    assert bool((cls == -1).all()) and not bool(reg.view(torch.int32).any())
    assert counts.cpu().tolist() == [0, 0, L.RPN_ERR_GT_COUNT, 0]
    assert ws_is_zero(ops)
    hc, hr, hb, hk, hcnt = ops.head_targets(rois, padded(hgt, 0, "copies", rois), padded_labels(lab, 0), n_rois=i32(300), want_keep=True, philox_state=st,
                                            status=status, n_gt=i32(n_gt), empty=empty, **kw)
    assert bool((hc == -1).all()) and bool((hk == -1).all()) and not bool(hr.view(torch.int32).any()) and not bool(hb.view(torch.int32).any())
    assert hcnt.cpu().tolist() == [0, 0, 0, L.HT_ERR_SHORT | L.HT_ERR_GT_COUNT]
    assert status.item() == L.HT_ERR_SHORT | L.HT_ERR_GT_COUNT and empty.item() == 1
    assert st.cpu().tolist()[1] == OFFSET + 2                                  # one value per call, as always
    assert "ground-truth" in " ".join(ops.describe_status(status.item()))
    # the next frame: two live boxes, from the same slot tensors
    st_ref = ops.philox_state(SEED, OFFSET + 2, DEV)
    ref_r = ops.rpn_targets(a, gt[:2].contiguous(), variant=variant, philox_state=st_ref)
    ref_h = ops.head_targets(rois, hgt[:2].contiguous(), lab[:2].contiguous(), n_rois=i32(300), want_keep=True, philox_state=st_ref, **kw)
    got_r = ops.rpn_targets(a, padded(gt, 2, "nan", a), variant=variant, philox_state=st, n_gt=i32(2))
    got_h = ops.head_targets(rois, padded(hgt, 2, "nan", rois), padded_labels(lab, 2), n_rois=i32(300), want_keep=True, philox_state=st, status=status,
                             n_gt=i32(2), empty=empty, **kw)
    assert all(same_bits(r, g_) for r, g_ in zip(ref_r + ref_h, got_r + got_h))
    assert empty.item() == 0 and torch.equal(st, st_ref)
    assert status.item() == L.HT_ERR_SHORT | L.HT_ERR_GT_COUNT                 # the status word IS sticky
    assert ws_is_zero(ops)


@pytest.mark.parametrize("variant", [0, 1])
def test_count_above_capacity_uses_the_capacity_and_writes_nothing_else(ops, L, variant):
    a, gt = rpn_data(2000)
    rois, hgt, lab = head_data()
    kw = HEAD_CONFIGS[variant]

    def case(g):
        st = g.place(ops.philox_state(SEED, OFFSET, DEV))
        empty, status = g.place(i32(5)), g.place(i32(0))
        cls, reg, counts = ops.rpn_targets(g.place(a), g.place(gt), variant=variant, philox_state=st, n_gt=g.place(i32(G_CAP + 5)))
        hc, hr, hb, hk, hcnt = ops.head_targets(g.place(rois), g.place(hgt), g.place(lab), n_rois=g.place(i32(300)), want_keep=True, philox_state=st,
                                                status=status, n_gt=g.place(i32(HG_CAP + 5)), empty=empty, **kw)
        return {"cls": cls, "reg": reg, "counts": counts, "head_cls": hc, "head_reg": hr, "head_rois": hb, "head_keep": hk, "head_counts": hcnt,
                "philox_state": st, "empty": empty, "status": status}
    out = G.run_both(case)[0]
    st = ops.philox_state(SEED, OFFSET, DEV)
    ref_r = ops.rpn_targets(a, gt, variant=variant, philox_state=st)
    ref_h = ops.head_targets(rois, hgt, lab, n_rois=i32(300), want_keep=True, philox_state=st, **kw)
    assert same_bits(out["cls"], ref_r[0]) and same_bits(out["reg"], ref_r[1])
    assert out["counts"].cpu().tolist() == ref_r[2].cpu().tolist()[:2] + [L.RPN_ERR_GT_COUNT, 0]
    for k, r in zip(("head_cls", "head_reg", "head_rois", "head_keep"), ref_h):
        assert same_bits(out[k], r), k
    ref_counts = ref_h[4].cpu().tolist()                                       # (total = 512 is short of candidates here: FRCNN_HT_ERR_SHORT in both)
    assert out["head_counts"].cpu().tolist() == ref_counts[:3] + [ref_counts[3] | L.HT_ERR_GT_COUNT]
    assert out["status"].item() == ref_counts[3] | L.HT_ERR_GT_COUNT and out["empty"].item() == 0 and torch.equal(out["philox_state"], st)


def test_c_abi_refusals(ops, L):
    lib, P = L.lib, lambda t: C.c_void_p(t.data_ptr())                          # noqa: E731
    a, gt = rpn_data(2000)
    rois, hgt, lab = head_data()
    n = i32(1)
    cls, reg, counts = torch.empty(2000, dtype=torch.int64, device=DEV), torch.empty(2000, 4, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    big = torch.zeros(L.workspace_bytes(L.OP_RPN_TARGETS, 2000, G_CAP), dtype=torch.uint8, device=DEV)

    def rpn(g_cap, ws, ws_bytes):
        return lib.frcnn_rpn_targets_n(0, P(a), 2000, P(gt), g_cap, P(n), None, 0, None, 0, 1, 2, None, P(cls), P(reg), P(counts), P(ws), ws_bytes, None)
    assert rpn(0, big, big.numel()) == -1 and b"G must be >= 1" in lib.frcnn_last_error()
    assert rpn(4097, big, big.numel()) == -1 and b"above limit 4096" in lib.frcnn_last_error()
    small = L.workspace_bytes(L.OP_RPN_TARGETS, 2000, 8)                        # sized for a smaller capacity: refused whatever *n_gt_dev says
    assert small < big.numel()
    assert rpn(G_CAP, big, small) == -3 and b"workspace" in lib.frcnn_last_error()       # FRCNN_ERR_WORKSPACE
    assert rpn(G_CAP, big, big.numel()) == 0
    torch.cuda.synchronize()
    assert counts.cpu().tolist()[2] == 0 and not bool(big[1536:1536 + 4096 * 64].any())

    hc, hr, hb, hcnt = torch.empty(128, dtype=torch.int64, device=DEV), torch.empty(128, 4, device=DEV), torch.empty(128, 4, device=DEV), \
        torch.zeros(4, dtype=torch.int32, device=DEV)

    def head(p_cap, g_cap):
        return lib.frcnn_head_targets_n(0, P(rois), None, p_cap, P(hgt), P(lab), g_cap, P(n), 1, 32, 128, None, 0, None, 0, 1, 2, None, P(hc), P(hr), P(hb),
                                        None, P(hcnt), None, None, None)
    assert head(300, 0) == -1 and b"G >= 1" in lib.frcnn_last_error()
    assert head(300, 4097) == -2 and b"above limit 4096" in lib.frcnn_last_error()       # FRCNN_ERR_UNSUPPORTED; the pointers are never followed
    assert head(4090, 7) == -2 and b"above limit 4096" in lib.frcnn_last_error()
    assert head(300, HG_CAP) == 0
    torch.cuda.synchronize()
    assert hcnt.cpu().tolist()[3] == 0
    with pytest.raises(ValueError, match="empty= goes with n_gt="):
        ops.head_targets(rois, hgt, lab, empty=i32(0))
    with pytest.raises(TypeError, match="n_gt must be torch.int32"):
        ops.rpn_targets(a, gt, n_gt=torch.tensor([3], device=DEV))


# ------------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("variant", [0, 1])
def test_one_captured_graph_serves_any_count(ops, variant):
    a, gt = rpn_data(24577 if variant else 2000)
    rois, hgt, lab = head_data()
    kw = HEAD_CONFIGS[variant]
    cap = HG_CAP
    s_gt, s_lab, n_gt, empty = gt[:cap].clone(), lab.clone(), i32(cap), i32(0)
    n_rois = i32(300)
    st = ops.philox_state(SEED, OFFSET, DEV)

    def both():
        r = ops.rpn_targets(a, s_gt, variant=variant, philox_state=st, n_gt=n_gt)
        h = ops.head_targets(rois, s_gt, s_lab, n_rois=n_rois, want_keep=True, philox_state=st, n_gt=n_gt, empty=empty, **kw)
        return r + h
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = both()
    st.copy_(ops.philox_state(SEED, 100, DEV))
    st_ref = ops.philox_state(SEED, 100, DEV)
    for k in (3, 17, 1):
        n_gt.fill_(k)
        s_gt.copy_(padded(gt[:cap], k, "copies", a))
        s_lab.copy_(padded_labels(lab, k))
        graph.replay()
        ref = ops.rpn_targets(a, gt[:k].contiguous(), variant=variant, philox_state=st_ref) + \
            ops.head_targets(rois, gt[:k].contiguous(), lab[:k].contiguous(), n_rois=n_rois, want_keep=True, philox_state=st_ref, **kw)
        for r, g_ in zip(ref, outs):
            assert same_bits(r, g_), k
        assert torch.equal(st, st_ref) and empty.item() == 0
    assert st.cpu().tolist()[1] == 100 + 6
