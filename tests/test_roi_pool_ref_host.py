"""CPU-only: tests/roi_pool_ref.py (the numpy restatement of RoIPool that tests/test_gpu_roi_pool_exact.py holds the HIP kernels to) equals
the C oracle in every bit of value and argmax on every named case, equals torchvision where that is installed, and every premise and
census that a case claims holds from the reference alone.  The launch plans the cases name are asserted here too: frcnn_roi_pool_plan
touches no device."""
import numpy as np
import pytest

import roi_pool_ref as rp
from oracle import oracle as orc

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the restatement = the oracle
@pytest.mark.parametrize("name", rp.ALL_CASES)
def test_reference_equals_the_c_oracle_in_every_bit(name):
    c = rp.case(name)
    for P in ((7, 5) if name.startswith(("geo", "values")) else (7,)):
        out, arg = rp.case_ref(name, P)
        out_o, arg_o = orc.roi_pool_fwd(c.feat, c.rois, P, P, c.scale)
        assert np.array_equal(arg, arg_o) and np.array_equal(bits(out), bits(out_o)), (name, P)
        g, _, _ = rp.case_bwd(name, P)                                       # asserts the exact regime
        assert np.array_equal(bits(g.astype(F)), bits(orc.roi_pool_bwd(c.go(P, P), arg_o, c.C, c.H, c.W))), (name, P)


@pytest.mark.parametrize("name", ["geo:halves/C3", "geo:scale16/C2", "geo:scale0.3/C2", "geo:sides/C2", "geo:artefact114/C2", "geo:kinds/C3",
                                  "plane:37x83", "rank:C2/24x24/R64"])
def test_reference_equals_torchvision(name):
    tv = pytest.importorskip("torchvision", reason="torchvision is not installed on this box: cross-check skipped (parity stays unpinned)")
    import torch
    c = rp.case(name)
    rois5 = torch.cat([torch.zeros(c.R, 1), torch.from_numpy(c.rois)], 1)
    got = tv.ops.roi_pool(torch.from_numpy(c.feat[None]), rois5, (7, 7), c.scale).numpy()
    assert np.array_equal(bits(got), bits(rp.case_ref(name)[0]))


# ---------------------------------------------------------------------------------------------- premises
def test_the_three_roundings_are_told_apart_by_the_halves():
    """A half has two neighbouring cells, so no single coordinate separates three rules: -0.5 separates half away (-1) from the other two
    (0), -1.5 separates floor(x + 0.5) (-1) from the other two (-2), 0.5 separates half even (0) from the other two (1)."""
    x = np.array([-1.5, -0.5, 0.5, 2.5], F)
    away, even, flo = rp.round_half_away(x), rp.round_half_even(x), rp.round_floor_half(x)
    assert away.tolist() == [-2, -1, 1, 3] and even.tolist() == [-2, 0, 0, 2] and flo.tolist() == [-1, 0, 1, 3]
    assert rp.round_half_away(F(0.49999997)) == 0 and rp.round_floor_half(F(0.49999997)) == 1          # why half away is not floor(x + 0.5)


def test_sides_57_and_114_end_one_cell_past_the_box_in_float32_only():
    for r in (57, 114):
        lo, hi = rp.bin_edges(10, r, 7)
        assert hi[-1] == 10 + r + 1 and lo[0] == 10
        assert int(np.ceil(7.0 * (r / 7.0))) == r                                                       # the same expression in float64
    n = sum(1 for r in range(1, 20001) if rp.bin_edges(0, r, 7)[1][-1] == r + 1)
    assert n == 581 and all(rp.bin_edges(0, r, 7)[1][-1] == r + 1 for r in (57, 114, 121, 228))


def test_bins_two_apart_overlap_only_below_seven_cells():
    """The rank scheme rests on this: for a side of at least P cells a pixel lies in at most two adjacent bins of an axis."""
    for r in range(7, 20001):
        lo, hi = rp.bin_edges(0, r, 7)
        assert (hi[:-2] <= lo[2:]).all(), r
    for r in range(1, 6):
        lo, hi = rp.bin_edges(0, r, 7)
        assert (hi[:-2] > lo[2:]).any(), r                                                              # small RoIs take the atomic branch
    lo, hi = rp.bin_edges(0, 6, 7)                                                                      # (a side of 6 does not overlap two apart
    assert (hi[:-2] <= lo[2:]).all()                                                                    #  either: the kernel's `>= 7` is on the safe side)


# ---------------------------------------------------------------------------------------------- censuses
@pytest.mark.parametrize("C", [2, 3])
def test_geometry_cases_are_not_degenerate(C):
    cen = {k: rp.geometry_census("geo:%s/C%d" % (k, C)) for k in rp.GEO_KINDS}
    for k in ("halves", "scale16"):
        assert cen[k]["half_even_differs"] and cen[k]["floor_half_differs"], k
        assert cen[k]["top"] and cen[k]["left"] and cen[k]["right"] and cen[k]["bottom"], (k, cen[k])
    a, b = rp.case_ref("geo:halves/C%d" % C), rp.case_ref("geo:scale16/C%d" % C)                       # the same cells through the scale
    assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
    assert cen["scale0.3"]["f64_product_differs"]                                                       # products rounded in fp32 decide cells
    assert cen["sides"]["empty"] == 0
    k = cen["kinds"]
    assert k["empty"] >= 5 * 49 and k["top"] and k["left"] and k["right"] and k["bottom"], k
    for name in ("artefact57", "artefact114"):
        assert rp.artefact_census("geo:%s/C%d" % (name, C)) >= 1
    arg = rp.case_ref("geo:kinds/C%d" % C)[1]
    assert (arg[7:11] == -1).all() and (arg[16] == -1).all() and (arg[12:16] >= 0).all()              # wholly outside; (W, H); the corners


def test_side_pairs_cover_the_bin_sizes():
    c = rp.case("geo:sides/C2")
    sides = set()
    for r in range(c.R):
        sw, sh, ew, eh = rp.roi_cells(c.rois[r], 1.0)
        sides.add((ew - sw + 1, eh - sh + 1))
    assert sides == {(w, h) for w in range(1, 15) for h in range(1, 15)} and {(6, 7), (7, 6), (7, 7), (8, 8), (14, 14), (1, 1)} <= sides


@pytest.mark.parametrize("C", [2, 3])
def test_value_cases_are_not_degenerate(C):
    for P in (7, 5):
        n = rp.values_census("values:/C%d" % C, P)
        assert n["nan_out"] == 0
        for k in ("all_nan", "all_neginf", "all_fltmin", "nan_skipped", "posinf", "plateau_first", "neg_zero", "pos_zero_won"):
            assert n[k] >= 1, (P, k, n)
    c = rp.case("values:/C%d" % C)
    out, arg = rp.case_ref(c.name)
    g, cnt, _ = rp.case_bwd(c.name)
    assert (arg == -1).any() and cnt.sum() == (arg >= 0).sum()                                          # the -1 bins add nothing


def test_rank_case_has_every_shape_of_shared_maximum_at_every_position():
    for C in (2, 6):
        shapes, pos = rp.rank_census("rank:C%d/24x24/R%d" % (C, rp.RANK_CENSUS_R))
        print("rank census C=%d:" % C, shapes, "positions min", pos.min())
        assert shapes.pop("other") == 0
        assert min(shapes.values()) >= 1, shapes
        assert pos.min() >= 1
    c = rp.case("rank:C2/24x24/R64")
    big = c.notes["big"]
    assert 8 <= (~big).sum() <= 32                                                                      # atomic RoIs among the rank ones ...
    mixed = [0 < (~big[w:64:8]).sum() < 8 for w in range(8)]                                            # wave w of 8 owns RoIs w, w + 8, ...: one batch of 16
    print('waves whose batch mixes rank and atomic RoIs:', sum(mixed))
    assert all(mixed)
    assert c.rois[:, 0].min() == -2 and c.rois[:, 1].min() == -2 and c.rois[:, 2].max() == 25 and c.rois[:, 3].max() == 25


# ---------------------------------------------------------------------------------------------- the plans the cases name
@pytest.fixture(scope="module")
def plan():
    from faster_rcnn_pytorch_amd import ops
    return ops.roi_pool_plan


def launch_geometry(C, R):
    """csrc/roi_pool.hip roi_pool_fwd_plan restated"""
    ncg = (C + 3) // 4
    S = min(max(-(-256 // ncg), -(-R // 256)), R)
    RB = -(-R // S)
    S = -(-R // RB)
    return S, RB, ncg * S <= 256


@pytest.mark.parametrize("C,R", rp.LAUNCH_CR)
def test_forward_launch_geometry_of_the_cases(plan, C, R):
    p = plan(C, 5, 7, R)
    assert p["fwd"] == "lds" and (p["S"], p["RB"], p["exclusive"]) == rp.LAUNCH_GEOMETRY[(C, R)] == launch_geometry(C, R)
    assert p["fwd_lds"] == (84 * 1024 if p["exclusive"] else 16 * 35 + 56 * p["RB"])
    assert plan(C, 5, 7, R, argmax16=False)["fwd"] == "lds"


def test_plans_at_the_plane_size_seams(plan):
    for H, W in rp.STAGING_SHAPES:
        assert plan(2, H, W, 7)["fwd"] == "lds" and plan(2, H, W, 7, argmax16=False)["fwd"] == "lds", (H, W)
    assert plan(2, *rp.LIMIT_SHAPE, 7)["fwd"] is None and plan(2, *rp.LIMIT_SHAPE, 7, argmax16=False)["fwd"] == "generic"
    assert plan(2, 16, 60, 7, (5, 5), argmax16=False)["fwd"] == "generic"
    for (H, W), form in rp.BWD16_SHAPES.items():
        p = plan(2, H, W, 7)
        assert p["bwd"] == form and p["bwd_lds"] == rp.BWD_LDS.get(("a16", (H, W)), p["bwd_lds"]), (H, W, p)
        assert p["rank_adds"] == (form in ("private8", "private4")) and not plan(2, H, W, 7, have_rois=False)["rank_adds"]
    for (H, W), form in rp.BWD32_SHAPES.items():
        p = plan(2, H, W, 7, argmax16=False)
        assert p["bwd"] == form and p["bwd_lds"] == rp.BWD_LDS.get(("i32", (H, W)), p["bwd_lds"]), (H, W, p)
    assert plan(2, 9, 9, 5, (17, 17), argmax16=False)["bwd"] == "one_channel"                          # a run longer than the workgroup
    assert plan(3, 32, 79, 7)["bwd"] == "shared_cb"                                                     # odd C
    for C, (H, W), R in rp.RANK_CASES:
        assert plan(C, H, W, R)["bwd"] == ("private8" if (H, W) == rp.RANK_NW8_HW else "private4")


def test_plan_honours_the_environment_switch_and_refuses_bad_arguments(plan, monkeypatch):
    from faster_rcnn_pytorch_amd import _lib
    monkeypatch.setenv("FRCNN_ROI_BWD_SHARED", "1")                                                     # (os.environ reaches the C library's getenv)
    assert plan(2, 24, 24, 64)["bwd"] == "shared_cb" and not plan(2, 24, 24, 64)["rank_adds"]
    monkeypatch.delenv("FRCNN_ROI_BWD_SHARED")
    assert plan(2, 24, 24, 64)["bwd"] == "private8"
    with pytest.raises(_lib.FrcnnError):
        plan(2, 24, 24, 0)
    with pytest.raises(_lib.FrcnnError):
        plan(2, 24, 24, 5, (5, 5), argmax16=True)
