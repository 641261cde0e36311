"""The box arithmetic of csrc/frcnn_common.h on the device, at its seams: det_expf (through ops.decode with unit anchors), det_log2f
(through ops.roi_level_map), iou_pair, decode4 / encode4 and prologue_one, against the oracle in every bit AND against the plain float64 /
exact references of tests/box_math_ref.py.  What ties the oracle's exp and log2 to the mathematics is tests/test_box_math_host.py.

Run on the GPU box:  python -m pytest tests/test_gpu_box_math_seams.py -m gpu -q -s   (-s shows the measured figures)
"""
import numpy as np
import pytest
import torch

import box_math_ref as R
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                        # a copy: the shared cases are read-only


def H(t):
    return t.detach().cpu().numpy()


# ============================================================================================ 1. exp
def test_exp_equals_the_oracle_on_E(ops):
    """Both cut-offs, every rounding seam of k, the whole subnormal-result range, 6.3 M magnitudes and the specials: every bit."""
    x = R.exp_inputs()
    t, a = R.exp_as_decode_rows(x)
    want = orc.decode(t, a)
    got = H(ops.decode(T(t), T(a)))
    assert R.same_bits(got, want), R.first_difference(got, want)
    g = R.exp_from_decode(got, len(x))
    tiny = np.float32(R.FLT_MIN)
    n_sub, n_sub_o = int(((g > 0) & (g < tiny)).sum()), int(((want[:, 2:] > 0) & (want[:, 2:] < tiny)).sum())
    print("exp on the device: %d inputs, %d nonzero subnormal results (oracle %d)" % (len(x), n_sub, n_sub_o))
    assert n_sub == n_sub_o and n_sub > 500000                         # a build that flushes subnormals to zero fails here by name
    (e_n, x_n), (e_s, x_s) = R.exp_maxima(x, g)                        # and the float64 bound holds for the kernel itself
    assert e_n <= R.EXP_BOUND_ULP and e_s <= R.EXP_BOUND_SUB, (e_n, x_n, e_s, x_s)
    nan = np.isnan(x)
    assert np.isnan(g[nan]).all() and (g[x == 0] == 1).all()
    assert (g[~nan & (x > np.float32(R.EXP_HI))] == np.inf).all() and (R.bits(g[~nan & (x < np.float32(R.EXP_LO))]) == 0).all()


# ============================================================================================ 2. the level mapper
@pytest.mark.parametrize("params", R.LEVEL_PARAMS)
def test_level_map_equals_the_oracle_and_obeys_the_rule(ops, params):
    rois = R.level_rois()
    want = orc.roi_level_map(rois, *params)
    got = H(ops.roi_level_map(T(rois), *params))
    bad = np.nonzero(got != want)[0]
    assert got.dtype == want.dtype and not len(bad), (params, rois[bad][:4], got[bad][:4], want[bad][:4])
    lo, hi, _, t64 = R.level_reference(rois, *params)
    ok = (got >= lo) & (got <= hi)
    assert ok.all(), (params, rois[~ok][:4], got[~ok][:4], lo[~ok][:4], hi[~ok][:4], t64[~ok][:4])
    deg = R.level_degenerate()
    for (name, _, end), l in zip(deg, got[-len(deg):]):
        if end is not None:
            assert l == (0 if end == "min" else params[1] - params[0]), (name, params, l)


# ============================================================================================ 3. IoU on exact data
def iou_all_ways(ops, s1, s2, what):
    """find_jaccard_overlap and both outputs of box_iou against the float64 reference and the oracle, every bit."""
    want, _, _ = R.iou_reference(s1, s2, R.IOU_EPS)
    got = H(ops.find_jaccard_overlap(T(s1), T(s2)))
    assert R.same_bits(got, want), (what, "jaccard", R.first_difference(got, want))
    assert R.same_bits(got, orc.pairwise_iou(s1, s2, R.IOU_EPS))
    want0, union, inter = R.iou_reference(s1, s2, 0.0)
    iou, second = ops.box_iou(T(s1), T(s2))
    iou, second = H(iou), H(second)
    assert R.same_bits(iou, want0), (what, "box_iou", R.first_difference(iou, want0))
    assert R.same_bits(iou, orc.pairwise_iou(s1, s2, 0.0))
    # what the second output holds, established from the two outputs themselves: the denominator of the first -- iou * second gives the
    # intersection back (exactly where the quotient is exact, to one rounding of the quotient elsewhere), so it is the union WITHOUT eps
    fin = np.isfinite(iou) & np.isfinite(second) & (second != 0)
    with np.errstate(invalid="ignore"):
        back = iou.astype(np.float64) * second.astype(np.float64)
    assert (np.abs(back - inter.astype(np.float64))[fin] <= 2.0 ** -24 * inter.astype(np.float64)[fin]).all(), what
    assert second.shape == iou.shape and R.same_bits(second, union), (what, "union", R.first_difference(second, union))
    return got, iou, second


@pytest.mark.parametrize("shape", R.IOU_SHAPES)
def test_iou_exact(ops, shape):
    s1, s2 = R.iou_sets(*shape)
    iou_all_ways(ops, s1, s2, shape)


def test_iou_named_rows(ops):
    named = R.iou_named()
    s1 = np.array([p for _, p, _, _ in named], np.float32)
    s2 = np.array([q for _, _, q, _ in named], np.float32)
    jac, iou, _ = iou_all_ways(ops, s1, s2, "named")
    stated = np.array([v for _, _, _, v in named], np.float32)
    d = np.diagonal(iou)
    assert R.same_bits(d, stated), [n for (n, _, _, _), a, b in zip(named, d, stated) if not R.same_bits([a], [b])]
    names = [n for n, _, _, _ in named]
    i = names.index("two identical empty boxes")
    assert np.isnan(iou[i, i]) and R.bits(jac)[i, i] == 0                                   # 0/0 without eps, 0/eps = +0 with it
    for n in ("NaN in set 1", "NaN in set 2"):                                             # as torch.max / torch.min propagate it
        j = names.index(n)
        assert np.isnan(iou[j, j]) and np.isnan(jac[j, j])
    assert np.isnan(iou[names.index("NaN in set 1"), :]).all() and np.isnan(iou[:, names.index("NaN in set 2")]).all()


# ============================================================================================ 4. codec on exact data
def test_decode_exact_and_the_contraction_witness(ops):
    t, a = R.decode_exact_case()
    want = R.decode_reference(t, a)
    got = H(ops.decode(T(t), T(a)))
    _, _, unfused, fused = R.witness_cxcy()
    assert got[0, 0] != np.float32(fused), "t.x * a.z + a.x was contracted into a fused multiply-add (-ffp-contract=off lost?)"
    assert got[0, 0] == np.float32(unfused)
    assert R.same_bits(got, want), R.first_difference(got, want)
    assert R.same_bits(got, orc.decode(t, a))


def test_encode_exact_and_log(ops):
    g, a = R.encode_exact_case()
    got = H(ops.encode(T(g), T(a)))
    want = R.encode_xy_reference(g, a)
    assert R.same_bits(got[:, :2], want), R.first_difference(got[:, :2], want)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert R.same_bits(got[:, :2], (g[:, :2] - a[:, :2]) / a[:, 2:])                   # numpy's binary32 division: x/0, 0/0
    assert np.isinf(got[-4:-2, 0]).all() and np.isnan(got[-2:, 0]).all()
    assert (R.bits(got[:-4, 2:]) == 0).all()                                                # log(1) = +0
    gl, al, _ = R.encode_log_case()
    out = H(ops.encode(T(gl), T(al)))
    err, z, specials_ok = R.log_check(gl[:, 2:], out[:, 2:])
    sub = (gl[:, 2:] > 0) & (gl[:, 2:] < np.float32(R.FLT_MIN))
    err_sub, z_sub, _ = R.log_check(gl[:, 2:][sub], out[:, 2:][sub])
    print("logf in encode4 on the device (%d inputs): %.4f ulp at g.z = %.9g (bits 0x%08X); over the %d subnormal ratios %.4f ulp at %.9g"
          % (2 * len(gl), err, z, R.bits1(z), int(sub.sum()), err_sub, z_sub))
    assert specials_ok
    assert err <= R.LOGF_BOUND_ULP_DEVICE, (err, z)


# ============================================================================================ prologue on exact data
@pytest.mark.parametrize("N", [1, 65, 777])
def test_prologue_exact(ops, N):
    reg, cls, anc = R.prologue_case(N)
    b_w, s_w, nv_w, keep = R.prologue_reference(reg, cls, anc, R.MIN_SIZE)
    b_o, s_o, nv_o = orc.proposal_prologue(reg, cls, anc, R.MIN_SIZE)
    b, s = ops.proposal_prologue(T(reg), T(cls), T(anc), R.MIN_SIZE)
    b, s = H(b), H(s)
    assert R.same_bits(b, b_w), (R.first_difference(b, b_w))
    assert R.same_bits(s, s_w), (R.first_difference(s, s_w))
    assert R.same_bits(b, b_o) and R.same_bits(s, s_o)
    assert int((s >= 0).sum()) == nv_w == nv_o
    boxes = R.prologue_box_cases()
    for i, (name, _, _, kept) in enumerate(boxes[:N]):                                     # logit pair 0 is (0, 0): the size rule alone decides
        assert (s[i] == 0.5) == kept, (name, s[i])
    if N == 777:
        for j, (c0, c1, sc) in enumerate(R.prologue_logit_cases()):                        # box case 0 is kept: the score shows
            assert R.same_bits([s[j * len(boxes)]], [sc]), (c0, c1, s[j * len(boxes)], sc)
        w = [n for n, _, _, _ in boxes].index("contraction witness")
        assert b[w, 2] != np.float32(R.witness_xyxy()[3]), "prologue_one: the decode was contracted into a fused multiply-add"
        assert b[w, 2] == np.float32(R.witness_xyxy()[2]) and b[w, 0] == 0


def test_region_proposal_with_planted_logit_pairs(ops):
    """16 x 16 x 9 anchors; (0, -inf), (-inf, 0), (0, 200), (-inf, -inf), (x, +inf), NaN ... planted in the logits: the whole stage
    returns the oracle's proposals from anchors in HBM and from anchors regenerated in registers."""
    reg, cls, planted = R.region_proposal_case()
    Hh = W = 256
    anchor = orc.anchor_grid(Hh, W)
    K = P = len(anchor)
    rois_o, src_o = orc.region_proposal(reg, cls, anchor, 1 / 1000, K, 0.7, P)
    grid = (Hh // 16, W // 16, 16, ops.anchor_base(), W, Hh)
    for anchors, g in ((T(anchor), None), (None, grid)):
        rois, cnt, src = ops.region_proposal(T(reg), T(cls), anchors, 1 / 1000, K, 0.7, P, grid=g, want_src=True)
        n = int(cnt.item())
        assert n == len(rois_o), (g is not None, n, len(rois_o))
        assert np.array_equal(H(src[:n]), src_o), (g is not None)
        assert R.same_bits(H(rois[:n]), rois_o), (g is not None)
    _, s_o, _ = orc.proposal_prologue(reg, cls, anchor, 1 / 1000)
    assert (s_o[src_o] >= 0).all() and np.isin(src_o, planted[s_o[planted] == 1]).any()
