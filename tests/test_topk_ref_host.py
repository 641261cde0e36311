"""CPU-only: tests/topk_ref.py (the numpy reference that tests/test_gpu_topk_seams.py holds csrc/topk.hip to) equals the C oracle and a
float64 lexsort wherever those are defined, differs from the oracle exactly where the order contract says so, and its host mirror of the
splitter sampling proves the premise of the GPU tests: every "unlucky sample" input makes the device rank a bucket of more than 1024
keys (or of exactly 1024 and 1025), and the seeded uniform inputs the suite has always used never do."""
import numpy as np
import pytest

import topk_ref as tr
from oracle import oracle as orc


def _seeded_inputs():
    rng = np.random.RandomState(0)
    uni = rng.rand(5000).astype(np.float32)
    uni[rng.rand(5000) < 0.1] = -1.0
    ties = (rng.randint(0, 40, 5000) / 64.0).astype(np.float32)
    ties[::11] = -1.0
    few = np.full(3000, -1.0, np.float32)
    few[rng.choice(3000, 200, replace=False)] = rng.rand(200).astype(np.float32)
    return {"uniform": uni, "heavy ties": ties, "all equal": np.full(300, 0.5, np.float32), "fewer live than K": few,
            "none live": np.full(70, -1.0, np.float32)}


@pytest.mark.parametrize("name", ["uniform", "heavy ties", "all equal", "fewer live than K", "none live"])
def test_reference_equals_the_c_oracle(name):
    s = _seeded_inputs()[name]
    for K in (1, 200, 3000, len(s)):
        idx, n = tr.topk(s, K)
        idx_o, sc_o = orc.topk_sorted(s, K)
        assert n == len(idx_o) and np.array_equal(idx, idx_o) and np.array_equal(s[idx], sc_o), (name, K)


def test_reference_equals_a_float64_lexsort_on_finite_scores():
    rng = np.random.RandomState(1)
    s = np.concatenate([rng.randn(4000), rng.randint(-3, 4, 3000) / 8.0, [3.4e38, -3.4e38, 1e-40, -1e-40, 1e-45]]).astype(np.float32)
    s = s[rng.permutation(len(s))]
    s[s == 0] = 0.0                                                           # no -0.0 here: float64 compares it equal to +0.0
    order = np.lexsort((np.arange(len(s)), -s.astype(np.float64)))
    idx, n = tr.topk(s, len(s), all_live=True)
    assert n == len(s) and np.array_equal(idx, order)
    live = order[s[order] >= 0]
    idx, n = tr.topk(s, 2500)
    assert n == 2500 and np.array_equal(idx, live[:2500])


def test_key32_is_the_total_order_on_bit_patterns():
    vals = np.concatenate([tr._f([0xFFC00000, 0xFF800001]), tr.NEG_SPECIALS[np.argsort(tr.NEG_SPECIALS, kind="stable")],
                           tr._f([0x80000000]), np.sort(tr.LIVE_SPECIALS[:-1]), tr._f([0x7F800001, 0x7FC00000])])
    k = tr.key32(vals).astype(np.int64)
    assert (np.diff(k) > 0).all(), "sign-set NaNs < -inf < ... < -0.0 < +0.0 < denormals < normals < +inf < sign-clear NaNs"
    assert k.min() >= 0 and k.max() <= 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- where the contract leaves the oracle
def test_contract_minus_zero_sorts_after_plus_zero():
    s = np.array([-0.0, 0.0, -0.0, 0.0, 0.5], np.float32)
    idx, n = tr.topk(s, 5)
    assert n == 5 and idx.tolist() == [4, 1, 3, 0, 2]                         # -0.0 is live (>= 0) and lies below +0.0
    assert orc.topk_sorted(s, 5)[0].tolist() == [4, 0, 1, 2, 3]               # the oracle's compare treats the zeros as a tie
    assert tr.topk(s, 5, all_live=True)[0].tolist() == [4, 1, 3, 0, 2]


def test_contract_nan_placement_when_all_live():
    s = np.array([0.25, 0, -np.inf, 0, np.inf, 0, -1.0], np.float32)
    s.view(np.uint32)[[1, 3, 5]] = [0xFFC00000, 0x7FC00000, 0x7F800001]
    idx, n = tr.topk(s, 7, all_live=True)
    assert n == 7 and idx.tolist() == [3, 5, 4, 0, 6, 2, 1]                   # sign-clear NaNs first (payload descending), the sign-set NaN last


def test_contract_no_nan_is_live_in_proposal_mode():
    s = np.array([0.25, 0, -np.inf, 0, np.inf, 0, -1.0], np.float32)
    s.view(np.uint32)[[1, 3, 5]] = [0xFFC00000, 0x7FC00000, 0x7F800001]
    idx, n = tr.topk(s, 7)
    assert n == 2 and idx.tolist() == [4, 0]
    assert tr.sort_keys(s).tolist() == tr.key32(np.array([0.25, -1, -1, -1, np.inf, -1, -1], np.float32)).tolist()


# ---------------------------------------------------------------------------------------------- the host mirror
def test_plan_gives_the_pairs_the_layout_stamp_records():
    """csrc/frcnn_layout.h stamps ss_plan at these sizes"""
    assert tr.plan(20646, 12000) == (512, 2)
    assert tr.plan(20646, 6000) == (512, 1)
    assert tr.plan(268569, 4000) == (2048, 1)
    assert tr.plan(65536, 65536) == (2048, 8)
    assert tr.plan(4096, 300) == (512, 1)
    assert tr.sample_positions(20646, 512)[[0, 1, 511]].tolist() == [0, 40, 20605]


def test_bucket_sizes_partition_the_input_in_rank_order():
    s = tr.case_scores("random", 20646, 12000, False)
    sizes, first, n_out = tr.bucket_sizes(s, 12000)
    assert sizes.sum() == len(s) and n_out == 12000
    idx, _ = tr.topk(s, len(s))                                               # bucket 0 is the best sizes[0] entries, and so on down the live ones
    comp = tr._composite(tr.sort_keys(s), np.arange(len(s)))
    assert (np.diff(comp[idx].astype(np.float64)) < 0).all()
    b = 0
    while first[b + 1] <= len(idx):
        lo, hi = comp[idx[first[b]:first[b + 1]]], comp[idx[first[b + 1]:first[b + 2]]] if first[b + 2] <= len(idx) else None
        assert hi is None or lo.min() > hi.max()
        b += 1


@pytest.mark.parametrize("all_live", [False, True])
@pytest.mark.parametrize("builder,N,K", tr.UNLUCKY_CASES)
def test_every_builder_makes_the_device_rank_a_bucket_above_1024_keys(builder, N, K, all_live):
    """The premise of test_gpu_topk_seams.py (a) / (b) / (e): without it those tests pass without entering the m > 1024 branch."""
    s, _, K = tr.case_inputs(builder, N, K, all_live)
    sizes, first, n_out = tr.bucket_sizes(s, K, all_live)
    tr.check_promise(builder, N, K, all_live, sizes, first, n_out)


def test_the_builders_give_the_sizes_they_name():
    s, _, _ = tr.low_samples(4096, 4096)
    assert tr.bucket_sizes(s, 4096, True)[0][0] == 4096 - 512 + 3             # the others, and the samples of rank 0, 1, 2 (the splitter included)
    s, _, _ = tr.high_samples(4096, 4096)
    sizes, first, _ = tr.bucket_sizes(s, 4096, True)
    assert sizes[255] == 3585 and first[255] == 511
    for N, K in ((4096, 4096), (8192, 8192), (20646, 12000), (65536, 65536), (70000, 4000)):
        s, _, _ = tr.exact_1024_1025(N, K)
        sizes = tr.bucket_sizes(s, K, True)[0]
        assert sizes[1] == 1024 and sizes[3] == 1025 and s.min() > 0 and s.max() <= 1, (N, K)
    s, _, _ = tr.periodic(4096, 4096)
    assert len(np.unique(s)) == 5 and np.array_equal(s, s[np.arange(4096) % 8])          # a function of i mod (N / S): the triangle's five levels


@pytest.mark.parametrize("N,K", [(20646, 12000), (20646, 6000), (268569, 4000), (268569, 2000), (100000, 2000), (40000, 10000)])
def test_the_seeded_uniform_inputs_of_the_suite_never_reach_the_branch(N, K):
    """The finding: the inputs of test_gpu_ops.py::test_topk_bit_exact (rebuilt here as that test builds them) keep every ranked bucket
    far below 1024 keys, so neither copy of the m > 1024 branch ran before test_gpu_topk_seams.py."""
    rng = np.random.RandomState(N + K)
    s = rng.rand(N).astype(np.float32)
    s[rng.rand(N) < 0.1] = -1.0
    assert tr.ranked(s, K).max() < 700


def test_the_heavy_tie_inputs_of_the_suite_never_reach_the_branch():
    rng = np.random.RandomState(3)
    s = (rng.randint(0, 2000, 150000) / 4096.0).astype(np.float32)
    s[::7] = -1.0
    assert tr.ranked(s, 3000).max() < 700
    s = (np.random.RandomState(7).randint(0, 40, 5000) / 64.0).astype(np.float32)
    s[::11] = -1.0
    assert tr.ranked(s, 3000).max() < 700


@pytest.mark.parametrize("which", ["low", "high"])
@pytest.mark.parametrize("K", [12000, 6000])
def test_the_proposal_logits_make_the_prologue_draw_an_unlucky_sample(which, K):
    anchor = orc.anchor_grid(600, 1000)
    reg, cls = tr.proposal_logits(len(anchor), K, which)
    _, s, _ = orc.proposal_prologue(reg, cls, anchor, 1 / 1000)
    sizes, first, n_out = tr.bucket_sizes(s, K)
    tr.check_promise(which + "_samples", len(s), K, False, sizes, first, n_out)
    assert sizes[0 if which == "low" else 255] > 15000


def test_seam_and_special_inputs_hold_what_they_name():
    for N in (300, 3000, 5000):
        s = tr.special_scores(N, True)
        u = s.view(np.uint32)
        for b in tr.NAN_BITS:
            assert (u == b).sum() == 5
        assert np.isnan(s[0]) and np.isnan(s[N - 1])
        for v in np.concatenate([tr.LIVE_SPECIALS, tr.NEG_SPECIALS]):
            where = np.nonzero(u == np.float32(v).view(np.uint32))[0]
            assert len(where) > 4 and (N < 3000 or len(np.unique(where // 1024)) > 1), (N, v)
        assert not np.isnan(tr.special_scores(N, False)).any()
    for kind in tr.SEAM_INPUTS:
        s = tr.seam_scores(kind, 4097)
        assert s.min() >= 0 and len(s) == 4097                                # all live until seam_dead() filters every seventh
    assert len(np.unique(tr.seam_scores("ascending", 65536))) == 65536 and len(np.unique(tr.seam_scores("twelve_values", 4095))) == 12
