"""The merge of evaluator shards on the host: the numpy restatement (tests/eval_merge_ref.py) against what the reference's own merge
selects (tests/golden/eval_merge.npz, written by tests/golden/make_golden_eval_merge.py from evaluation/coco_eval.py:161-180), its
associativity, and the refusals of the C entry points, which are decided before anything is launched and so need no device."""
import ctypes as C

import numpy as np
import pytest

import eval_merge_ref as R


@pytest.fixture(scope="module")
def cases(golden):
    return R.golden_cases(golden("eval_merge"))


def test_golden_file_holds_every_kind(golden):
    z = golden("eval_merge")
    want = {"sampler_padding_w2", "sampler_padding_w3", "sampler_padding_w8", "duplicate_inside_one_shard", "empty_shard", "single_shard",
            "all_shards_identical", "negative_ids", "extreme_ids"}
    assert set(z["kinds"].tolist()) == want and (z["kind_counts"] >= 1).all()


def test_restatement_selects_what_the_reference_merge_selects(cases):
    for name, (ids, merged_ids, selected) in cases.items():
        kept = R.kept_occurrences(ids)
        kept_ids = np.array([ids[w][r] for w, r in kept], np.int32)
        order = np.argsort(kept_ids, kind="stable")             # the reference returns the ids ascending (np.unique)
        assert np.array_equal(kept_ids[order], merged_ids), name
        assert np.array_equal(np.array(kept, np.int64).reshape(-1, 2)[order], selected), name
        assert kept == sorted(kept), name


@pytest.mark.parametrize("fw", [1, 4])
def test_restatement_records_ledger_and_counter(cases, fw):
    """The merged store of the restatement against a second, slower formulation: per kept occurrence the shard's own slice."""
    rng = np.random.RandomState(5 + fw)
    for name, (ids, _, selected) in cases.items():
        shards = [R.make_shard(rng, s, fw, 6, shard=w) for w, s in enumerate(ids)]
        m = R.merge(shards)
        sel = sorted((int(w), int(r)) for w, r in selected)
        assert m["n_images"] == len(sel) and m["led_image"].tolist() == [int(ids[w][r]) for w, r in sel], name
        pos = 0
        for k, (w, r) in enumerate(sel):
            b, e = shards[w]["led_range"][r]
            assert m["led_range"][k].tolist() == [pos, pos + e - b], name
            for col in R.COLUMNS:
                assert np.array_equal(m[col][pos:pos + e - b].view(np.uint8), shards[w][col][b:e].view(np.uint8)), (name, col)
            pos += e - b
        assert m["n_records"] == pos == len(m["score"])
        assert np.array_equal(m["counter"], sum((shards[w]["led_delta"][r].astype(np.int64) for w, r in sel), np.zeros(6, np.int64))), name
        assert (m["led_range"][1:, 0] == m["led_range"][:-1, 1]).all()


@pytest.mark.parametrize("seed", range(6))
def test_merge_is_associative(seed):
    rng = np.random.RandomState(100 + seed)
    fw = 1 if seed % 2 else 4
    a, b, c, d = (R.make_shard(rng, rng.randint(-6, 12, rng.randint(0, 25)), fw, 4, shard=w) for w in range(4))
    flat = R.merge([a, b, c, d])
    R.same(R.merge([R.merge([a, b]), c, d]), flat, "((a b) c d)")
    R.same(R.merge([a, R.merge([b, c]), d]), flat, "(a (b c) d)")
    R.same(R.merge([R.merge([a, b]), R.merge([c, d])]), flat, "((a b) (c d))")
    R.same(R.merge([R.merge([a, b, c, d])]), flat, "idempotent")


# ---------------------------------------------------------------------------------------------------------------- the C ABI's refusals
@pytest.fixture(scope="module")
def L():
    from faster_rcnn_pytorch_amd import _lib
    return _lib


INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
P_SRC, P_DST, P_LED, P_TAIL, P_WS = range(5, 16), range(16, 21), range(22, 25), range(26, 32), 32


def _merge_args(L, W=2, SR=8, SI=4, FW=1, CW=3, RC=32, IC=8):
    """Arguments of frcnn_eval_merge that pass every check: distinct, 4 KiB aligned addresses 1 MiB apart (never dereferenced: the
    refusals under test are decided before a launch)."""
    ptrs = [0x10000000 + 0x100000 * k for k in range(26)]
    need = L.workspace_bytes(L.OP_EVAL_MERGE, W * SR, W * SI)
    return [W, SR, SI, FW, CW] + ptrs[:11] + ptrs[11:16] + [RC] + ptrs[16:19] + [IC] + ptrs[19:25] + [ptrs[25], need, None]


def _refused(L, args, code, word):
    rc = L.lib.frcnn_eval_merge(*args)
    msg = L.lib.frcnn_last_error().decode()
    assert rc == code and "eval_merge" in msg and word in msg, (rc, msg)


def test_merge_workspace_bytes(L):
    assert L.OP_EVAL_MERGE == 14
    small, big = L.workspace_bytes(L.OP_EVAL_MERGE, 8 * 4096, 8 * 64), L.workspace_bytes(L.OP_EVAL_MERGE, 8 * 65536, 8 * 640)
    assert 0 < small < big
    assert big >= 8 * 65536 + 8 * 640 + 8 * 2 * 8 * 640             # a flag byte per record and per row, a table slot per two occurrences
    assert L.workspace_bytes(L.OP_EVAL_MERGE, 1 << 31, 1) == 0 and L.workspace_bytes(L.OP_EVAL_MERGE, 1, 1 << 30) == 0
    assert L.workspace_bytes(L.OP_EVAL_MERGE, 0, 0) > 0


def test_merge_refuses_null_pointers(L):
    for i in list(P_SRC) + list(P_DST) + list(P_LED) + list(P_TAIL) + [P_WS]:
        a = _merge_args(L)
        a[i] = None
        _refused(L, a, INVALID, "NULL")


def test_merge_refuses_shard_counts_and_capacities(L):
    for W in (0, -1, 65):
        a = _merge_args(L)
        a[0] = W
        _refused(L, a, UNSUPPORTED, "shards outside 1 .. 64")
    for i in (1, 2, 21, 25):                                        # shard records, shard images, record_capacity, image_capacity
        a = _merge_args(L)
        a[i] = -4
        _refused(L, a, INVALID, "negative capacity")
    a = _merge_args(L)
    a[1] = 6
    _refused(L, a, INVALID, "multiple of 4")
    for cw in (0, 1021):
        a = _merge_args(L)
        a[4] = cw
        _refused(L, a, UNSUPPORTED, "counter words")
    _refused(L, _merge_args(L, W=64, SR=1 << 26), UNSUPPORTED, "2^31")


def test_merge_refuses_flags_width(L):
    for fw in (0, 2, 3, 5):
        a = _merge_args(L)
        a[3] = fw
        _refused(L, a, INVALID, "flags_width")


def test_merge_refuses_short_workspace(L):
    a = _merge_args(L)
    a[33] -= 1
    _refused(L, a, WORKSPACE, "workspace")
    a[33] = 0
    _refused(L, a, WORKSPACE, "workspace")


def test_merge_refuses_misaligned_buffers(L):
    for i in list(P_SRC)[:5] + list(P_DST):
        a = _merge_args(L)
        a[i] += 4
        _refused(L, a, INVALID, "16-byte aligned")
    for i in (11, 13, 14, 23, 26, 27, 28, 30, 31):                  # the int64 buffers
        a = _merge_args(L)
        a[i] += 4
        _refused(L, a, INVALID, "8-byte aligned")


def test_merge_refuses_overlapping_buffers(L):
    a = _merge_args(L)
    a[16] = a[5] + 16                                               # rec_score inside sh_score [2, 8]
    _refused(L, a, INVALID, "overlaps a shard buffer")
    a = _merge_args(L)
    a[17] = a[16] + 64                                              # rec_label inside rec_score [32]
    _refused(L, a, INVALID, "two destination buffers overlap")
    a = _merge_args(L)
    a[26] = a[P_WS] + 256                                           # the counter inside the workspace
    _refused(L, a, INVALID, "overlaps the workspace")
    a = _merge_args(L)
    a[P_WS] = a[8] + 16                                             # the workspace on a shard column
    _refused(L, a, INVALID, "overlaps the workspace")
    a = _merge_args(L)
    a[27] = a[13]                                                   # the cursor on the shards' record counts
    _refused(L, a, INVALID, "overlaps a shard buffer")


def test_ledger_append_refusals(L):
    ptrs = [0x10000000 + 0x100000 * k for k in range(10)]
    ok = ptrs[:3] + [3] + ptrs[3:8] + [16] + ptrs[8:10] + [None]
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 10, 11):
        a = list(ok)
        a[i] = None
        assert L.lib.frcnn_eval_ledger_append(*a) == INVALID and b"NULL" in L.lib.frcnn_last_error()
    a = list(ok)
    a[9] = 0
    assert L.lib.frcnn_eval_ledger_append(*a) == INVALID and b"image_capacity" in L.lib.frcnn_last_error()
    for cw in (0, 1021):
        a = list(ok)
        a[3] = cw
        assert L.lib.frcnn_eval_ledger_append(*a) == UNSUPPORTED and b"counter words" in L.lib.frcnn_last_error()


def test_binding_knows_the_new_error_bits(L):
    assert (L.EVAL_ERR_LEDGER_OVERFLOW, L.EVAL_ERR_SHARD_TRUNCATED, L.EVAL_MERGE_MAX_SHARDS) == (16, 32, 64)
    assert C.sizeof(C.c_int64) == 8
