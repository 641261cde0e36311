"""CPU only: the premises of tests/test_gpu_box_math_seams.py, checked on the oracle (oracle/frcnn_oracle.c).

The GPU suite asserts that the kernels of csrc/frcnn_common.h equal the oracle in every bit.  The oracle's exp and log2 are the same
operation sequence as the kernels' by construction, so what THIS file asserts -- the oracle against numpy's float64 exp / log2 / log,
against exact references on exact data and against the level rule -- is what ties the kernels to the mathematics.  Every measured
figure is printed before it is asserted (pytest -s shows them); the constants live in tests/box_math_ref.py and docs/PARITY.md.
"""
import numpy as np
import pytest

import box_math_ref as R
from oracle import oracle as orc


def oracle_exp(x):
    """orc_expf over an array through oracle.decode with unit anchors (columns 2, 3 = orc_expf(t) * 1.0f)."""
    t, a = R.exp_as_decode_rows(x)
    return R.exp_from_decode(orc.decode(t, a), len(x))


# ============================================================================================ 1. exp
def test_exp_decode_route_is_the_scalar_function():
    """The bulk route returns what the scalar entry point returns, on the windows round both cut-offs and the specials."""
    x = np.concatenate([R.ulp_window(R.EXP_HI, 8), R.ulp_window(R.EXP_LO, 8), R.ulp_window(0.5 * R.LN2, 8), R.exp_specials()])
    assert R.same_bits(oracle_exp(x), orc.expf(x))


def test_exp_vs_float64_on_E():
    x = R.exp_inputs()
    got = oracle_exp(x)
    (e_n, x_n), (e_s, x_s) = R.exp_maxima(x, got)
    print("orc_expf on E (%d inputs): %.4f ulp at x = %.9g (bits 0x%08X); %.4f units of 2^-149 at x = %.9g (bits 0x%08X)"
          % (len(x), e_n, x_n, R.bits1(x_n), e_s, x_s, R.bits1(x_s)))
    assert e_n <= R.EXP_BOUND_ULP and e_s <= R.EXP_BOUND_SUB
    # the recorded maxima are what this set gives (docs/PARITY.md holds the same figures)
    assert abs(e_n - R.EXP_MEASURED_ULP) < 1e-3 and abs(e_s - R.EXP_MEASURED_SUB) < 1e-3
    # the set does reach the subnormal results, both seams of every k and both cut-offs
    sub = (got > 0) & (got < np.float32(R.FLT_MIN))
    assert sub.sum() > 500000
    assert (x > np.float32(R.EXP_HI)).sum() > 64 and (x < np.float32(R.EXP_LO)).sum() > 64


def test_exp_exact_values():
    x = R.exp_inputs()
    got = oracle_exp(x)
    nan = np.isnan(x)
    assert nan.sum() == 3 and np.isnan(got[nan]).all()                                       # NaN in, NaN out (payload, sign: any)
    assert (got[x == 0] == 1.0).all() and (x == 0).sum() == 2                                # exp(+-0) == 1
    assert (got[~nan & (x > np.float32(R.EXP_HI))] == np.inf).all()                          # above the upper cut-off, +inf included
    below = ~nan & (x < np.float32(R.EXP_LO))
    assert (R.bits(got[below]) == 0).all()                                                   # below the lower cut-off: +0, -inf included
    assert got[x == np.inf] == np.inf and R.bits(got[x == -np.inf]) == 0
    assert (got[~nan] >= 0).all()
    s = orc.expf(np.array([89.0, -104.0, -200.0, 0.0, -0.0], np.float32))
    assert np.isinf(s[0]) and (s[1:3] == 0).all() and (s[3:] == 1).all()
    # monotone over the ordered part of E where two results differ by more than the asserted error: a wrong k at a seam is a factor 2
    fin = ~nan & np.isfinite(x)
    o = np.argsort(x[fin], kind="stable")
    g = got[fin][o].astype(np.float64)
    assert (g[1:] >= g[:-1] * (1 - 2 * R.EXP_BOUND_ULP * 2.0 ** -23) - R.EXP_BOUND_SUB * 2 * R.DENORM).all()


# ============================================================================================ 2. log2
def test_log2_array_route_is_the_scalar_function():
    a = np.concatenate([R.ulp_window(R.SQRT2_CUT, 4), R.ulp_window(1.0, 4), R.from_bits([1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF]),
                        np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan], np.float32)])
    assert R.same_bits(orc.log2f_array(a), orc.log2f(a))


def test_log2_exact_on_powers_of_two_and_specials():
    a, e = R.powers_of_two()
    got = orc.log2f_array(a)
    assert len(a) == 277 and (a[:23] < np.float32(R.FLT_MIN)).all() and a[0] == np.float32(R.DENORM)
    assert np.array_equal(got, e), (a[got != e][:4], got[got != e][:4])                      # subnormals: the e = -24 offset
    s = orc.log2f_array(np.array([0.0, -0.0, np.inf, -1.0, -np.inf, np.nan], np.float32))
    assert s[0] == -np.inf and s[1] == -np.inf and s[2] == np.inf and np.isnan(s[3:]).all()
    assert np.isnan(orc.log2f_array(R.from_bits([0x80000001])))                              # a negative subnormal is negative


def test_log2_vs_float64():
    narrow, wide = R.log2_inputs()
    assert narrow.min() == 1 / 16 and narrow.max() == 16 and len(narrow) > 1500000
    worst = []
    for name, a in (("[1/16, 16]", narrow), ("every exponent", wide)):
        err, units = R.log2_errors(a, orc.log2f_array(a))
        i = int(np.argmax(units))
        print("orc_log2f on %s (%d inputs): %.4e absolute = %.4f units at a = %.9g (bits 0x%08X)"
              % (name, len(a), err[i], units[i], a[i], R.bits1(a[i])))
        assert units[i] <= R.LOG2_BOUND_UNITS
        worst.append((err[i], units[i]))
    assert abs(worst[0][1] - R.LOG2_MEASURED_UNITS) < 1e-3 and abs(worst[0][0] - R.LOG2_MEASURED_ABS) < 1e-10


# ============================================================================================ the level rule
def check_levels(lv, rois, params, who):
    """Every row: the level is the one float64 gives, or, within `band` of an integer, one of the two on either side."""
    lo, hi, band, t64 = R.level_reference(rois, *params)
    ok = (lv >= lo) & (lv <= hi)
    assert ok.all(), (who, params, rois[~ok][:4], lv[~ok][:4], lo[~ok][:4], hi[~ok][:4], t64[~ok][:4])
    return lo, hi, band, t64


@pytest.mark.parametrize("params", R.LEVEL_PARAMS)
def test_level_rule_on_the_oracle(params):
    rois = R.level_rois()
    lv = orc.roi_level_map(rois, *params)
    lo, hi, band, t64 = check_levels(lv, rois, params, "oracle")
    k_min, k_max = params[0], params[1]
    undecided = lo != hi
    # sanity of the derived band: it comes out near 1e-6 where t is in [4, 8), and the rows on which the oracle differs from float64
    # all lie well inside it
    chain = ~np.isnan(t64)
    mid = chain & (t64 > 4.5) & (t64 < 7.5)
    want = np.clip(np.floor(np.where(chain, t64, 0)), k_min, k_max).astype(np.int32) - k_min
    differs = chain & (lv != want)
    dist = np.abs(t64 - np.rint(t64))
    print("level rule %s: %d rows, %d within the band of an integer, %d where the oracle differs from floor(t64), farthest %.3e; band %.3e .. %.3e"
          % (params, len(rois), undecided.sum(), differs.sum(), dist[differs].max() if differs.any() else 0.0, band[mid].min(), band[mid].max()))
    assert 1.0e-6 < band[mid].min() and band[mid].max() < 1.6e-6
    assert differs.sum() > 100                                            # the set does hold rows where binary32 and float64 part ways
    assert not differs.any() or dist[differs].max() < band[mid].min()
    assert undecided.sum() < 0.9 * len(rois)                              # and rows that the rule decides outright
    assert set(lv.tolist()) == (set(range(4)) if k_min == 2 else set(range(8)))   # both ends of the clamp and every level between


def test_level_degenerate_rows_on_the_oracle():
    deg = R.level_degenerate()
    rois = np.array([r for _, r, _ in deg], np.float32)
    assert np.array_equal(R.level_rois()[-len(deg):], rois, equal_nan=True)
    for params in R.LEVEL_PARAMS:
        lv = orc.roi_level_map(rois, *params)
        lo, hi, _, _ = R.level_reference(rois, *params)
        for (name, _, end), l, a, b in zip(deg, lv, lo, hi):
            if end is not None:
                assert a == b == (0 if end == "min" else params[1] - params[0]), name
            assert a <= l <= b, (name, params, l, a, b)


# ============================================================================================ 3. IoU on exact data
@pytest.mark.parametrize("shape", R.IOU_SHAPES)
def test_iou_exact_on_the_oracle(shape):
    s1, s2 = R.iou_sets(*shape)
    assert R.is_dyadic(s1, 10) and R.is_dyadic(s2, 10)
    for eps in (R.IOU_EPS, 0.0):
        want, union, inter = R.iou_reference(s1, s2, eps)
        got = orc.pairwise_iou(s1, s2, eps)
        assert R.same_bits(got, want), (shape, eps, R.first_difference(got, want))
    # exactness premise: union and intersection are multiples of 2^-20 below 4
    assert R.is_dyadic(union, 20) and R.is_dyadic(inter, 20) and np.nanmax(np.abs(union[np.isfinite(union)])) <= 2.0


def test_iou_named_rows_on_the_oracle():
    named = R.iou_named()
    s1 = np.array([p for _, p, _, _ in named], np.float32)
    s2 = np.array([q for _, _, q, _ in named], np.float32)
    for eps in (R.IOU_EPS, 0.0):
        want, _, _ = R.iou_reference(s1, s2, eps)
        got = orc.pairwise_iou(s1, s2, eps)
        assert R.same_bits(got, want), (eps, R.first_difference(got, want))
    d = np.diagonal(orc.pairwise_iou(s1, s2, 0.0))
    stated = np.array([v for _, _, _, v in named], np.float32)
    assert R.same_bits(d, stated), [n for (n, _, _, _), a, b in zip(named, d, stated) if not R.same_bits([a], [b])]
    i = [n for n, _, _, _ in named].index("two identical empty boxes")
    assert np.isnan(d[i]) and R.bits(orc.pairwise_iou(s1, s2, R.IOU_EPS))[i, i] == 0           # 0/0 without eps, +0 with it


# ============================================================================================ 4. codec and prologue on exact data
def test_decode_exact_and_the_contraction_witness_on_the_oracle():
    t, a = R.decode_exact_case()
    want = R.decode_reference(t, a)
    # premise: apart from the witness nothing rounds -- the float64 value of t * a.z + a.x is a binary32 number
    exact = t.astype(np.float64)[1:, :2] * a.astype(np.float64)[1:, 2:] + a.astype(np.float64)[1:, :2]
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact) and np.array_equal(want[1:, :2], exact.astype(np.float32))
    _, _, unfused, fused = R.witness_cxcy()
    assert want[0, 0] == np.float32(unfused) != np.float32(fused)
    assert float(t[0, 0]) * float(a[0, 2]) + float(a[0, 0]) == fused                           # what one rounding would give
    got = orc.decode(t, a)
    assert R.same_bits(got, want), R.first_difference(got, want)


def test_encode_exact_and_log_on_the_oracle():
    g, a = R.encode_exact_case()
    got = orc.encode(g, a)
    assert R.same_bits(got[:, :2], R.encode_xy_reference(g, a)), R.first_difference(got[:, :2], R.encode_xy_reference(g, a))
    with np.errstate(invalid="ignore", divide="ignore"):
        f32 = (g[:, :2] - a[:, :2]) / a[:, 2:]                                                  # numpy's binary32 division
    assert R.same_bits(got[:, :2], f32)
    assert np.isinf(got[-4:-2, 0]).all() and np.isnan(got[-2:, 0]).all()
    assert (R.bits(got[:-4, 2:]) == 0).all()                                                     # log(1) = +0
    gl, al, n_special = R.encode_log_case()
    out = orc.encode(gl, al)
    err, z, specials_ok = R.log_check(gl[:, 2:], out[:, 2:])
    print("logf in orc_encode (%d inputs): %.4f ulp at g.z = %.9g (bits 0x%08X)" % (2 * len(gl), err, z, R.bits1(z)))
    assert specials_ok and err <= R.LOGF_BOUND_ULP_HOST                                          # measured: R.LOGF_MEASURED_HOST (the C library's, so not pinned)


@pytest.mark.parametrize("N", [1, 65, 777])
def test_prologue_exact_on_the_oracle(N):
    reg, cls, anc = R.prologue_case(N)
    b_w, s_w, nv_w, keep = R.prologue_reference(reg, cls, anc, R.MIN_SIZE)
    b_o, s_o, nv_o = orc.proposal_prologue(reg, cls, anc, R.MIN_SIZE)
    assert R.same_bits(b_o, b_w), R.first_difference(b_o, b_w)
    assert R.same_bits(s_o, s_w), R.first_difference(s_o, s_w)
    assert nv_o == nv_w == int((s_o >= 0).sum())
    if N >= len(R.prologue_box_cases()):
        for i, (name, _, _, kept) in enumerate(R.prologue_box_cases()):
            assert bool(keep[i]) == kept, name
    if N == 777:
        logits = R.prologue_logit_cases()
        nb = len(R.prologue_box_cases())
        for j, (c0, c1, s) in enumerate(logits):                                                 # box case 0 is kept: the score shows
            assert R.same_bits([s_o[j * nb]], [s]), (c0, c1, s_o[j * nb], s)
        assert (s_o == 0).sum() > 0 and (s_o == 1).sum() > 0 and (s_o == 0.5).sum() > 0 and (s_o == -1).sum() > 0
        w = [n for n, _, _, _ in R.prologue_box_cases()].index("contraction witness")
        assert b_o[w, 2] == np.float32(R.witness_xyxy()[2]) != np.float32(R.witness_xyxy()[3]) and b_o[w, 0] == 0


def test_region_proposal_case_reaches_the_planted_scores():
    """The planted logit pairs decide which anchors the oracle's proposal stage may return: none of the filtered ones ever."""
    reg, cls, planted = R.region_proposal_case()
    anchor = orc.anchor_grid(256, 256)
    assert len(anchor) == len(reg) == 2304
    _, s, nv = orc.proposal_prologue(reg, cls, anchor, 1 / 1000)
    assert (s[planted] == -1).sum() >= 16 * 7 and (s[planted] == 0).sum() > 0 and (s[planted] == 1).sum() > 0
    rois, src = orc.region_proposal(reg, cls, anchor, 1 / 1000, 2304, 0.7, 2304)
    assert len(src) > 100 and (s[src] >= 0).all() and (np.diff(s[src]) <= 0).all()
