"""CPU proof of tests/roi_align_ref.py before any kernel is looked at: the float64 reference equals the C oracle bit for bit on the exact
(dyadic) cases and holds it inside the derived bound on general data; and every premise the GPU file (tests/test_gpu_roi_align_exact.py)
relies on is true of the data -- the 2^24 limit, the level map, the list lengths, segment counts and chunk trips each seam case claims to
reach, the plan's coarsening, the item-block counts on either side of the resident workgroup count, and the tiles nobody touches."""
import numpy as np
import pytest

import roi_align_ref as ra
from oracle import oracle as orc

CH = 4          # channels of the oracle comparisons (channels are independent; the reference runs at the cases' full C)


@pytest.mark.parametrize("name", ra.EXACT_CASES)
def test_exact_case_premise_and_oracle_equal_ref64_in_every_bit(name):
    c = ra.case(name)
    worst = ra.check_premise(name)
    assert worst < 2 ** 24
    if len(c.shapes) > 1:
        assert np.array_equal(orc.roi_level_map(c.rois), c.level)
    ref = ra.case_ref(name)
    rng = np.random.RandomState(5)
    nch = min(CH, c.C)
    for l, ((h, w), s) in enumerate(zip(c.shapes, c.scales)):
        o = _orc_bwd(c, nch, h, w, s, l)
        assert np.array_equal(o.astype(np.float64), ref[l][0][:nch]), (name, l)
        assert np.array_equal(o.view(np.uint32), ref[l][0][:nch].astype(np.float32).view(np.uint32)), (name, l)
        feat = rng.randint(-8, 9, (2, h, w)).astype(np.float32)
        fo = orc.roi_align_fwd(feat, c.rois, c.PH, c.PH, s, c.SR, c.aligned, c.level, l)
        assert np.array_equal(fo.astype(np.float64), ra.fwd64(feat, c.rois, s, c.aligned, c.level, l, c.PH, c.SR)), (name, l)


def _orc_bwd(c, nch, h, w, s, l):
    """orc.roi_align_bwd takes PH from grad_out's shape."""
    return orc.roi_align_bwd(c.go[:, :nch], (nch, h, w), c.rois, s, c.SR, c.aligned, c.level, l)


@pytest.mark.parametrize("name", ["pyr", "one"])
def test_general_data_oracle_within_the_derived_bound(name):
    c = ra.general_case(name)
    if len(c.shapes) > 1:
        assert set(c.level.tolist()) == {0, 1, 2, 3}
    ref = ra.general_ref(name)
    for l, ((h, w), s) in enumerate(zip(c.shapes, c.scales)):
        n_l = int((c.level == l).sum())
        o = orc.roi_align_bwd(c.go[:, :CH], (CH, h, w), c.rois, s, 2, False, c.level, l).astype(np.float64)
        g, a = ref[l][0][:CH], ref[l][1][:CH]
        assert np.array_equal(o == 0, a == 0), "zero patterns differ"
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(a > 0, np.abs(o - g) / (2.0 ** -24 * a), 0.0)
        print("PARITY oracle general %s level %d: n_l %d, worst err %.2f x 2^-24 absgrad (bound %d)" % (name, l, n_l, q.max(), ra.bound_units(n_l)))
        assert (np.abs(o - g) <= ra.bound_units(n_l) * 2.0 ** -24 * a).all()


def test_dyadic_set_of_the_issue_600_rois_four_levels():
    """600 RoIs, sides 7 * 2^j (j = 2..7), corners on multiples of 2 px, dOut integers in [-8, 8], scales 1/4 .. 1/32."""
    c = ra.case("b2b:")
    assert c.R == 600 and set(c.level.tolist()) == {0, 1, 2, 3} and c.unit >= 2.0 ** -12
    sides = np.concatenate([c.rois[:, 2] - c.rois[:, 0], c.rois[:, 3] - c.rois[:, 1]])
    assert set(np.log2(sides / 7).tolist()) == {2.0, 3.0, 4.0, 5.0, 6.0, 7.0}
    assert (c.rois % 2 == 0).all() and np.abs(c.go).max() == 8
    # RoIs partly outside on each side, wholly outside, and clamped at the last row / column
    Wi, Hi = ra.IMG_WH
    r = c.rois
    assert ((r[:, 0] < 0) & (r[:, 2] > 0)).any() and ((r[:, 1] < 0) & (r[:, 3] > 0)).any()
    assert ((r[:, 2] > Wi) & (r[:, 0] < Wi)).any() and ((r[:, 3] > Hi) & (r[:, 1] < Hi)).any()
    assert (r[:, 0] > Wi + 16).any() and (r[:, 1] > Hi + 16).any() and (r[:, 2] < -32).any()


@pytest.mark.parametrize("n", ra.SEG_LENGTHS)
def test_seam_single_tile_list_lengths_and_segments(n):
    c = ra.case("seg:%d" % n)
    (cnt, _), = ra.tile_lists(c.rois, c.shapes, c.scales, c.aligned, c.level)
    assert cnt.shape == (1, 1) and cnt[0, 0] == n == c.R and c.C == 32
    split, items, cap, segs = ra.plan(cnt.ravel(), c.R)
    assert split == ra.RS_SPLIT and items <= cap
    want = {1: 1, 32: 1, 33: 2, 64: 2, 65: 3, 1024: 32, 1025: 32, 2080: 32, 2081: 32}[n]
    assert len(segs[0]) == want and sum(segs[0]) == n
    if n == 1024:
        assert set(segs[0]) == {32}
    if n == 2080:
        assert set(segs[0]) == {65}                         # second trip of the chunk loop, with ONE entry
    if n == 2081:
        assert sorted(set(segs[0])) == [65, 66]
    if n >= 2080:
        assert min(segs[0]) > ra.RS_CHUNK
        assert np.abs(c.go).max() <= 2
    if n == 1025:
        assert max(segs[0]) == 33 and max(segs[0]) <= ra.RS_CHUNK


@pytest.mark.parametrize("R", ra.CHUNK_R)
def test_seam_lists_kernel_chunks_share_tiles(R):
    c = ra.case("chunk:%d" % R)
    first = ra.tile_lists(c.rois[:256], c.shapes, c.scales, False, c.level[:256])[0][0]
    last0 = (R - 1) // 256 * 256
    if last0 == 0:
        last0 = R - 1                                   # one chunk (R <= 256): its last lanes
    tail = np.zeros(R, bool); tail[last0:] = True
    lv = np.where(tail, 0, 9).astype(np.int32)          # only the last chunk's RoIs
    last = ra.tile_lists(c.rois, c.shapes, c.scales, False, lv)[0][0]
    assert ((first > 0) & (last > 0)).any() and (last > 0).sum() >= 1
    assert ((last > 0) <= (first > 0)).all()            # every tile the last chunk reaches also holds first-chunk RoIs


def test_seam_mixed_records_and_in_kernel_tables_share_lists():
    c = ra.case("mixed:")
    (cnt, span), = ra.tile_lists(c.rois, c.shapes, c.scales, False, c.level)
    small = np.array([span[r] <= ra.RA_MAXT for r in range(c.R)])
    assert small.sum() >= 40 and (~small).sum() >= 20
    # interleaved in index order on shared tiles: some tile's list alternates between the kinds several times
    best = 0
    for ty in range(cnt.shape[0]):
        for tx in range(cnt.shape[1]):
            kinds = [small[r] for r in range(c.R)
                     if (lambda f: f[0] // 16 <= ty <= f[1] // 16 and f[2] // 8 <= tx <= f[3] // 8)(ra.footprint(c.rois[r], 50, 84, 1.0 / 16, False))]
            best = max(best, int(np.sum(np.diff(np.array(kinds, int)) != 0)))
    assert best >= 8


def test_seam_plan_coarsens():
    c = ra.case("coarsen:")
    (cnt, _), = ra.tile_lists(c.rois, c.shapes, c.scales, False, c.level)
    tiles = cnt.size
    assert tiles == 44
    assert sum(-(-int(n) // 32) for n in cnt.ravel()) > tiles + 15 * c.R // 32 + 1      # the issue's condition: the loop must double at least once
    split, items, cap, _ = ra.plan(cnt.ravel(), c.R)
    assert split >= 2 * ra.RS_SPLIT and items <= cap


def test_seam_grid_order_item_blocks_on_both_sides_of_the_resident_count_and_untouched_tiles():
    for name, above in (("pyr:64", False), ("pyr:128", True)):
        c = ra.case(name)
        lists = ra.tile_lists(c.rois, c.shapes, c.scales, False, c.level)
        counts = np.concatenate([cn.ravel() for cn, _ in lists])
        _, items, cap, _ = ra.plan(counts, c.R)
        n_cg = -(-c.C // ra.RT_CB)
        assert items <= cap
        if above:
            assert cap * n_cg > ra.RESIDENT_MAX        # whatever the occupancy: fill blocks sit INSIDE the grid
        else:
            assert cap * n_cg < ra.RESIDENT_MIN        # the fill blocks come last
        assert (counts == 0).sum() >= 10 and set(c.level.tolist()) == {0, 1, 2, 3}
        cn0 = lists[0][0]
        a0 = ra.case_ref(name)[0][1]
        ty, tx = np.argwhere(cn0 == 0)[0]
        assert (a0[:, ty * 16:ty * 16 + 16, tx * 8:tx * 8 + 8] == 0).all()
    c = ra.case("pyr_empty:")
    assert (ra.tile_lists(c.rois, c.shapes, c.scales, False, c.level)[0][0] == 0).all() and (ra.case_ref("pyr_empty:")[0][1] == 0).all()


def test_footprint_contains_every_nonzero_weight():
    """The tile model's footprint is the kernel's hit test; a weight outside it would be a contribution no tile gathers."""
    for name in ("pyr:64", "aligned:pyr", "shape:1x3"):
        c = ra.case(name)
        for r in range(0, c.R, 3):
            (H, W), s = c.shapes[c.level[r]], c.scales[c.level[r]]
            Wy, Wx, _ = ra.roi_weights(c.rois[r], H, W, s, c.aligned)
            y0, y1, x0, x1 = ra.footprint(c.rois[r], H, W, s, c.aligned)
            ys, xs = np.flatnonzero(Wy.any(1)), np.flatnonzero(Wx.any(1))
            assert len(ys) == 0 or (ys[0] >= y0 and ys[-1] <= y1)
            assert len(xs) == 0 or (xs[0] >= x0 and xs[-1] <= x1)


def test_register_and_generic_cases_are_what_they_claim():
    for Cc in ra.REG_PATH_C:
        assert ra.case("regC:%d" % Cc).C % 32 != 0
    assert ra.case("dma64:").C % 32 == 0
    for PH, SR in ra.GENERIC:
        c = ra.case("generic:%d/%d" % (PH, SR))
        assert (c.PH, c.SR) != (7, 2)
        for r in range(c.R):
            *_, gh, gw, cnt = ra.roi_geom(c.rois[r], c.scales[0], PH, PH, SR, False)
            assert int(cnt) & (int(cnt) - 1) == 0 and (SR != 0 or gh == gw)
        if SR == 0:
            assert len({ra.roi_geom(c.rois[r], c.scales[0], PH, PH, SR, False)[4] for r in range(c.R)}) >= 3
