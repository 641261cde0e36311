"""The image ledger of the device evaluators and the merge of their shards (csrc/eval_merge.hip, evaluation.merge_shards) on the device,
against the restatements: tests/eval_ref.py and tests/coco_eval_ref.py for what a frame contributes, tests/eval_merge_ref.py (pinned to
the reference's own merge by tests/test_eval_merge_host.py) for the merge.  Everything is integer bookkeeping and verbatim copies, so
every comparison is bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import coco_eval_ref
import eval_merge_ref as R
import eval_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = (0.3, 0.5, 0.75)
NC = 7                                                          # 6 object classes
KINDS = ("voc", "coco")


def _source_constant(name):
    txt = open(os.path.join(ROOT, "faster_rcnn_pytorch_amd", "csrc", "eval_merge.hip")).read()
    return int(re.search(r"#define %s (\d+)" % name, txt).group(1))


SCAN_BLOCK = _source_constant("MERGE_SCAN_BLOCK")               # records per workgroup of the compaction
ROW_BLOCK = _source_constant("MERGE_ROW_BLOCK")                 # ledger rows per workgroup


def _mods():
    from faster_rcnn_pytorch_amd import _lib, evaluation, ops
    return evaluation, ops, _lib


def _ev(kind, num_classes=NC, record_capacity=1 << 12, image_capacity=256, **kw):
    evaluation = _mods()[0]
    if image_capacity is not None:
        kw["image_capacity"] = image_capacity
    if kind == "voc":
        return evaluation.DetectionEvaluator(num_classes, THR, record_capacity=record_capacity, gt_capacity=16, device=DEV, **kw)
    return evaluation.CocoDetectionEvaluator(num_classes, record_capacity=record_capacity, gt_capacity=16, device=DEV, **kw)


def _words(kind, num_classes=NC):
    return (num_classes - 1) * (1 if kind == "voc" else 4)


def _dets(f, cap=64, count=None):
    ops = _mods()[1]
    D = len(f["labels"])
    boxes = torch.full((cap, 4), float("nan"), dtype=torch.float32)
    labels = torch.full((cap,), 10 ** 6, dtype=torch.int32)
    scores = torch.full((cap,), 2.0, dtype=torch.float32)
    boxes[:D] = torch.from_numpy(np.ascontiguousarray(f["boxes"], np.float32).reshape(-1, 4))
    labels[:D] = torch.from_numpy(np.ascontiguousarray(f["labels"], np.int32))
    scores[:D] = torch.from_numpy(np.ascontiguousarray(f["scores"], np.float32))
    cnt = torch.tensor([D if count is None else count], dtype=torch.int32)
    return ops.Detections(boxes.to(DEV), labels.to(DEV), scores.to(DEV), cnt.to(DEV), None, None, None)


class _Feeder(object):
    """update() of one evaluator frame by frame, the frame's tensors built once per frame dict."""
    def __init__(self, kind, ev):
        evaluation = _mods()[0]
        self.kind, self.ev = kind, ev
        self.gt = (evaluation.GroundTruth if kind == "voc" else evaluation.CocoGroundTruth)(16, DEV)

    def feed(self, f, image_id=None, count=None):
        iid = f["image_id"] if image_id is None else image_id
        if self.kind == "voc":
            self.gt.set(f["gt_boxes"], f["gt_labels"], f["gt_difficult"], (f["w"], f["h"]), iid)
        else:
            self.gt.set(f["gt_boxes"], f["gt_labels"], f["gt_iscrowd"], f["gt_area"], orig_wh=(f["w"], f["h"]), image_id=iid)
        self.ev.update(_dets(f, count=count), self.gt)


def _contribution(kind, f):
    """(records, counter delta) of one frame by the protocol's restatement."""
    if kind == "voc":
        return len(f["labels"]), eval_ref.npos_of([f], NC)
    r = coco_eval_ref.run([f], NC)
    return len(r["records"]["label"]), np.asarray(r["npig"], np.int64).reshape(-1)


_frames, _special = {}, {}


def _pool(kind):
    """40 seeded frames of at most 64 detections and 16 ground truths, made once and never modified.  _special[kind] = (a frame that
    has lost its detections, a frame that has lost its ground truths): the first two frames that had both."""
    if kind not in _frames:
        if kind == "voc":
            fr = eval_ref.make_set(411, n_images=40, num_classes=NC, max_gt=16, max_det=64)
        else:
            fr = coco_eval_ref.make_set(412, n_images=40, num_classes=NC, max_det=64, max_gt=16)
        assert max(len(f["labels"]) for f in fr) <= 64 and max(len(f["gt_labels"]) for f in fr) <= 16
        full = [k for k, f in enumerate(fr) if k != 7 and _contribution(kind, f)[0] > 0 and _contribution(kind, f)[1].any()]
        for k in ("boxes", "labels", "scores"):
            fr[full[0]][k] = fr[full[0]][k][:0]
        for k in [k for k in fr[full[1]] if k.startswith("gt_")]:
            fr[full[1]][k] = fr[full[1]][k][:0]
        _frames[kind], _special[kind] = fr, (full[0], full[1])
    return _frames[kind]


def _host(ev):
    """The evaluator's live content as a shard dict of host arrays (tests/eval_merge_ref.py) plus its counter."""
    s = ev.state()
    out = {k: s[k].cpu().numpy() for k in ("score", "label", "image_id", "flags", "led_image", "led_range", "led_delta")}
    out.update(order=s[ev._COLUMN].cpu().numpy(), n_records=s["n_records"], n_images=s["n_images"], error=int(s["error"].item()),
               counter=s[ev._COUNTER[0]].reshape(-1).cpu().numpy())
    return out


def _as_state(ev, sh):
    """A numpy shard as a state() dict of evaluators like `ev`."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    s = {k: t(sh[k]) for k in ("score", "label", "image_id", "flags", "led_image", "led_range", "led_delta")}
    s[ev._COLUMN] = t(sh["order"])
    s[ev._COUNTER[0]] = torch.zeros_like(ev._counter)
    s.update(n_records=int(sh["n_records"]), n_images=int(sh["n_images"]), error=torch.tensor([int(sh["error"])], dtype=torch.int32, device=DEV),
             **ev._config())
    return s


def _load(ev, sh):
    """Puts a numpy shard into the evaluator's own buffers, in place (what a captured graph reads)."""
    ev.reset()
    n, m = len(sh["score"]), len(sh["led_image"])
    for dst, k in zip(ev._records(), R.COLUMNS):
        dst[:n].copy_(torch.from_numpy(np.ascontiguousarray(sh[k])))
    ev.led_image[:m].copy_(torch.from_numpy(sh["led_image"]))
    ev.led_range[:m].copy_(torch.from_numpy(sh["led_range"]))
    ev.led_delta[:m].copy_(torch.from_numpy(sh["led_delta"]))
    ev.cursor.fill_(int(sh["n_records"]))
    ev.led_count.fill_(int(sh["n_images"]))
    ev.error.fill_(int(sh["error"]))


def _poison(ev):
    """0xFF in every integer buffer and NaN in the scores: what the merge does not write stays visible."""
    ev.rec_score.fill_(float("nan"))
    for t in (ev.rec_label, ev.rec_image, ev._rec_order, ev.rec_flags, ev.led_image, ev.led_range, ev.led_delta, ev._counter, ev.cursor, ev.led_count,
              ev.error, ev._snap_cursor, ev._snap_counter):
        t.fill_(-1)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _merge_and_check(kind, shards, record_capacity=1 << 12, image_capacity=256, num_classes=NC):
    """Merges numpy shards through state() dicts into a poisoned evaluator and holds it to the restatement, bit for bit."""
    ev = _ev(kind, num_classes, record_capacity, image_capacity)
    _poison(ev)
    ev.merge_shards([_as_state(ev, s) for s in shards])
    want = R.merge(shards, record_capacity, image_capacity)
    got = _host(ev)
    R.same(got, want, kind)
    assert _bits(ev._snap_counter.cpu().numpy(), want["counter"]) and int(ev._snap_cursor.item()) == want["n_records"]
    # nothing is written behind the merged content
    n, m = min(want["n_records"], record_capacity), min(want["n_images"], image_capacity)
    assert bool(torch.isnan(ev.rec_score[n:]).all()) and bool((ev.rec_flags[n:] == -1).all()) and bool((ev.rec_label[n:] == -1).all())
    assert bool((ev.led_image[m:] == -1).all()) and bool((ev.led_range[m:] == -1).all()) and bool((ev.led_delta[m:] == -1).all())
    return ev, want


# ------------------------------------------------------------------------------------------------------------ 1. the ledger
@pytest.mark.parametrize("kind", KINDS)
def test_ledger_rows_of_40_updates(kind):
    frames = _pool(kind)
    ev = _ev(kind)
    fd = _Feeder(kind, ev)
    ids = [int(v) for v in 200 - 13 * np.arange(40)]            # descending, negative from the 17th: the ledger keeps the order of update
    ids[11], ids[12] = -1, int(np.iinfo(np.int32).min)
    want_range, want_delta, pos = [], [], 0
    for k, f in enumerate(frames):
        aborted = k == 7
        fd.feed(f, image_id=ids[k], count=-1 if aborted else None)      # an upstream abort: the frame records nothing and counts nothing
        n, d = (0, np.zeros(_words(kind), np.int64)) if aborted else _contribution(kind, f)
        want_range.append((pos, pos + n))
        want_delta.append(d)
        pos += n
    got = _host(ev)
    _, _, L = _mods()
    assert got["n_images"] == 40 and got["n_records"] == pos and got["error"] == L.EVAL_ERR_UPSTREAM_ABORT
    assert got["led_image"].dtype == np.int32 and got["led_image"].tolist() == ids
    assert got["led_range"].dtype == np.int64 and got["led_range"].tolist() == [list(r) for r in want_range]
    assert got["led_delta"].dtype == np.int32 and np.array_equal(got["led_delta"], np.array(want_delta))
    no_det, no_gt = _special[kind]                              # the frames without detections / without ground truth
    assert want_range[no_det][0] == want_range[no_det][1] and np.any(want_delta[no_det])
    assert want_range[no_gt][0] < want_range[no_gt][1] and not np.any(want_delta[no_gt])
    assert np.array_equal(got["led_delta"].astype(np.int64).sum(0), got["counter"]) and got["counter"].sum() > 0
    assert np.array_equal(got["image_id"], np.repeat(np.array(ids, np.int32), [e - b for b, e in want_range]))
    ev.reset()
    z = _host(ev)
    assert z["n_images"] == 0 and z["n_records"] == 0 and int(ev._snap_cursor.item()) == 0 and not bool(ev._snap_counter.any())
    fd.feed(frames[0], image_id=5)                              # after a reset the first row starts at slot 0 with the whole counter
    z = _host(ev)
    assert z["led_range"].tolist() == [[0, _contribution(kind, frames[0])[0]]] and np.array_equal(z["led_delta"][0], z["counter"])


# ------------------------------------------------------------------------------------------------------------ 2. merge == one evaluator
def _same_summary(kind, a, b):
    keys = ("ap", "map", "npos", "tp", "fp") if kind == "voc" else ("stats", "precision", "recall", "npig")
    for k in keys:
        assert _bits(a[k], b[k]), k
    assert a["n_records"] == b["n_records"]


@pytest.mark.parametrize("kind", KINDS)
def test_merge_of_golden_patterns_equals_one_evaluator(kind, golden):
    frames = _pool(kind)
    for name, (ids, merged_ids, _) in R.golden_cases(golden("eval_merge")).items():
        frame_of = {int(v): frames[k % len(frames)] for k, v in enumerate(merged_ids)}      # one frame per distinct image
        shards = []
        for s in ids:
            fd = _Feeder(kind, _ev(kind))
            for v in s:
                fd.feed(frame_of[int(v)], image_id=int(v))
            shards.append(fd.ev)
        one = _Feeder(kind, _ev(kind, image_capacity=None))
        for v in merged_ids:
            one.feed(frame_of[int(v)], image_id=int(v))
        merged = _ev(kind)
        _poison(merged)
        merged.merge_shards([s.state() if k % 2 else s for k, s in enumerate(shards)])      # evaluators and state() dicts alike
        _same_summary(kind, merged.summarize(), one.ev.summarize())
        ra, rb = merged.records_sorted(), one.ev.records_sorted()
        assert sorted(ra) == sorted(rb)
        for k in ra:
            assert _bits(ra[k], rb[k]), (name, k)
        want = R.merge([_host(s) for s in shards], merged.record_capacity, merged.image_capacity)
        R.same(_host(merged), want, name)
        assert sorted(want["led_image"].tolist()) == merged_ids.tolist(), name


# ------------------------------------------------------------------------------------------------------------ 3. compaction seams
def _split(rng, total, parts):
    cuts = np.sort(rng.randint(0, total + 1, parts - 1))
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(int).tolist()


@pytest.mark.parametrize("kind", KINDS)
def test_compaction_at_the_scan_block_seams(kind):
    """Shards of 0, 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1 and 2 * SCAN_BLOCK + 1 records behind a donor shard; in every shard
    the images alternate between new ids (kept) and the donor's (dropped); the last shard repeats the one before it and goes entirely."""
    assert SCAN_BLOCK == 1024 and ROW_BLOCK == 256
    rng = np.random.RandomState(31)
    fw, cw = (1 if kind == "voc" else 4), _words(kind)
    shards = [R.make_shard(rng, [1000, 1001, 1002], fw, cw, shard=0)]
    for w, total in enumerate((0, 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1), 1):
        ids = [10 * w, 1000, 10 * w + 1, 1001, 10 * w + 2, 1002]
        shards.append(R.make_shard(rng, ids, fw, cw, shard=w, counts=_split(rng, total, 6)))
        assert shards[-1]["n_records"] == total
    shards.append(R.make_shard(rng, shards[-1]["led_image"], fw, cw, shard=7, counts=_split(rng, SCAN_BLOCK + 3, 6)))
    _, want = _merge_and_check(kind, shards, record_capacity=1 << 13)
    assert want["n_images"] == 3 + 6 * 3 and 0 < want["n_records"] < sum(s["n_records"] for s in shards)
    # one long image across two scan blocks, dropped in one shard and kept in the next; and kept records that end exactly on a block
    a = R.make_shard(rng, [1, 2, 3], fw, cw, shard=0, counts=[3, SCAN_BLOCK + 5, SCAN_BLOCK - 8])
    b = R.make_shard(rng, [2, 4, 1], fw, cw, shard=1, counts=[7, 2 * SCAN_BLOCK, 1])
    _merge_and_check(kind, [a, b], record_capacity=1 << 13)
    _merge_and_check(kind, [b, a], record_capacity=1 << 13)


@pytest.mark.parametrize("kind", KINDS)
def test_64_tiny_shards_and_more_rows_than_a_row_block(kind):
    rng = np.random.RandomState(64)
    fw, cw = (1 if kind == "voc" else 4), _words(kind)
    shards = [R.make_shard(rng, rng.randint(-5, 25, rng.randint(0, 4)), fw, cw, max_records=3, shard=w) for w in range(64)]
    _, want = _merge_and_check(kind, shards)
    assert 20 <= want["n_images"] <= 30
    evaluation = _mods()[0]
    with pytest.raises(ValueError, match="outside 1 .. 64"):
        ev = _ev(kind)
        ev.merge_shards([_as_state(ev, s) for s in shards] + [_as_state(ev, shards[0])])
    with pytest.raises(ValueError, match="outside 1 .. 64"):
        _ev(kind).merge_shards([])
    assert evaluation.MAX_CLASSES == 256
    # 2 * ROW_BLOCK + 1 rows in one shard: the ledger's own compaction crosses its block seams
    ids = rng.randint(0, 300, 2 * ROW_BLOCK + 1)
    _merge_and_check(kind, [R.make_shard(rng, ids, fw, cw, max_records=2, shard=0), R.make_shard(rng, ids[::-1], fw, cw, max_records=2, shard=1)],
                     image_capacity=1024)


# ------------------------------------------------------------------------------------------------------------ 4. dedupe seams
def _table_slots(n_occurrences):
    ts = 64
    while ts < 2 * n_occurrences:
        ts *= 2
    return ts


@pytest.mark.parametrize("kind", KINDS)
def test_ids_that_collide_in_the_table(kind):
    """Two shards of 16 rows: 64 slots, slot = id mod 64.  Every id below lands on slot 5 or 6, from both ends of the int32 range."""
    rng = np.random.RandomState(5)
    fw, cw = (1 if kind == "voc" else 4), _words(kind)
    ts = _table_slots(2 * 16)
    assert ts == 64
    i32 = np.iinfo(np.int32)
    pool = [5 + ts * k for k in (-3, -2, -1, 0, 1, 2, 3, 1000)] + [6 + ts * k for k in (-1, 0, 1)] + [int(i32.min) + 5, int(i32.max) - 63 + 5, -1, 0,
                                                                                                  int(i32.min), int(i32.max)]
    assert all((v % ts) in (5, 6) for v in pool[:13]) and all(i32.min <= v <= i32.max for v in pool)
    a = R.make_shard(rng, [pool[i] for i in rng.randint(0, len(pool), 16)], fw, cw, shard=0)
    b = R.make_shard(rng, [pool[i] for i in rng.permutation(len(pool))[:16]], fw, cw, shard=1)
    _, want = _merge_and_check(kind, [a, b])
    assert want["n_images"] == len(set(a["led_image"].tolist()) | set(b["led_image"].tolist()))


@pytest.mark.parametrize("kind", KINDS)
def test_4096_occurrences_of_64_ids(kind):
    rng = np.random.RandomState(4096)
    fw, cw = (1 if kind == "voc" else 4), _words(kind)
    ids64 = rng.randint(-2 ** 31, 2 ** 31, 64).astype(np.int64)
    shards = [R.make_shard(rng, ids64[rng.randint(0, 64, 512)], fw, cw, max_records=2, shard=w) for w in range(8)]
    _, want = _merge_and_check(kind, shards, image_capacity=128)
    assert want["n_images"] == 64 and sorted(want["led_image"].tolist()) == sorted(ids64.tolist())


# ------------------------------------------------------------------------------------------------------------ 5. overflow
@pytest.mark.parametrize("kind", KINDS)
def test_record_overflow_keeps_counting(kind):
    evaluation, _, L = _mods()
    rng = np.random.RandomState(77)
    fw, cw = (1 if kind == "voc" else 4), _words(kind)
    shards = [R.make_shard(rng, range(20 * w, 20 * w + 12), fw, cw, shard=w, counts=[5] * 12) for w in range(3)]
    ev, want = _merge_and_check(kind, shards, record_capacity=101)
    assert want["n_records"] == 180 and len(want["score"]) == 101 and int(ev.cursor.item()) == 180 and want["error"] == 0
    with pytest.raises(L.FrcnnError, match="record store is full"):
        ev.summarize()
    # a shard that had lost records itself says so after the merge
    cut = dict(shards[0], **{k: shards[0][k][:40] for k in R.COLUMNS})
    ev, want = _merge_and_check(kind, [cut, shards[1]])
    assert want["error"] == L.EVAL_ERR_SHARD_TRUNCATED and want["n_records"] == 40 + 60
    with pytest.raises(L.FrcnnError, match="lost records"):
        ev.summarize()


@pytest.mark.parametrize("kind", KINDS)
def test_ledger_overflow_at_append_and_at_merge(kind):
    evaluation, _, L = _mods()
    frames = _pool(kind)
    fd = _Feeder(kind, _ev(kind, image_capacity=3))
    for k in range(5):
        fd.feed(frames[k], image_id=k)
    h = _host(fd.ev)
    assert h["n_images"] == 5 and len(h["led_image"]) == 3 and h["error"] == L.EVAL_ERR_LEDGER_OVERFLOW
    assert h["led_image"].tolist() == [0, 1, 2] and h["n_records"] == sum(_contribution(kind, f)[0] for f in frames[:5])
    with pytest.raises(L.FrcnnError, match="image_capacity = 3"):
        fd.ev.summarize()
    rng = np.random.RandomState(78)
    fw, cw = (1 if kind == "voc" else 4), _words(kind)
    shards = [R.make_shard(rng, range(10 * w, 10 * w + 6), fw, cw, shard=w) for w in range(3)]
    ev, want = _merge_and_check(kind, shards, image_capacity=16)
    assert want["n_images"] == 18 and want["error"] == L.EVAL_ERR_LEDGER_OVERFLOW and int(ev.led_count.item()) == 18
    assert np.array_equal(want["counter"], sum(s["led_delta"].astype(np.int64).sum(0) for s in shards))      # the rows past the ledger count too
    with pytest.raises(L.FrcnnError, match="image_capacity = 16"):
        ev.summarize()


@pytest.mark.parametrize("kind", KINDS)
def test_append_only_merge_refuses_a_ledger(kind):
    a, b = _ev(kind), _ev(kind)
    with pytest.raises(ValueError, match="merge_shards"):
        a.merge(b)
    plain = _ev(kind, image_capacity=None)
    with pytest.raises(ValueError, match="image_capacity"):
        plain.merge_shards([a])
    with pytest.raises(ValueError, match="image_capacity"):
        a.merge_shards([plain])
    with pytest.raises(ValueError, match="image_capacity"):
        a.merge_shards([plain.state()])
    with pytest.raises(ValueError, match="differ"):
        a.merge_shards([_ev(kind, num_classes=NC + 1)])


# ------------------------------------------------------------------------------------------------------------ 6. associativity
@pytest.mark.parametrize("kind", KINDS)
def test_merge_is_associative_on_the_device(kind):
    rng = np.random.RandomState(9)
    fw, cw = (1 if kind == "voc" else 4), _words(kind)
    a, b, c = (R.make_shard(rng, rng.randint(-4, 14, 20), fw, cw, shard=w) for w in range(3))
    ev = _ev(kind)
    sa, sb, sc = (_as_state(ev, s) for s in (a, b, c))
    flat = _host(_ev(kind).merge_shards([sa, sb, sc]))
    ab = _ev(kind).merge_shards([sa, sb])
    bc = _ev(kind).merge_shards([sb, sc])
    R.same(_host(_ev(kind).merge_shards([ab, sc])), flat, "(a b) c")
    R.same(_host(_ev(kind).merge_shards([sa, bc.state()])), flat, "a (b c)")
    R.same(_host(ab.merge_shards([ab, sc])), flat, "into one of its own shards")
    R.same(flat, R.merge([a, b, c]), "restatement")
    # the merged evaluator goes on: a further update appends behind the merge and its ledger row starts there
    frames = _pool(kind)
    fd = _Feeder(kind, ab)
    fd.feed(frames[0], image_id=777)
    h = _host(ab)
    n, d = _contribution(kind, frames[0])
    assert h["n_images"] == flat["n_images"] + 1 and h["led_range"][-1].tolist() == [flat["n_records"], flat["n_records"] + n]
    assert np.array_equal(h["led_delta"][-1], d) and np.array_equal(h["counter"], flat["counter"] + d)


# ------------------------------------------------------------------------------------------------------------ 7. capture
@pytest.mark.parametrize("kind", KINDS)
def test_one_captured_merge_replays_on_other_contents_and_counts(kind):
    rng = np.random.RandomState(17)
    fw, cw = (1 if kind == "voc" else 4), _words(kind)
    a, b, dst = _ev(kind, record_capacity=4096, image_capacity=64), _ev(kind, record_capacity=2048, image_capacity=48), _ev(kind, record_capacity=8192)
    contents = [(R.make_shard(rng, rng.randint(0, 30, 40), fw, cw, shard=0, max_records=60), R.make_shard(rng, rng.randint(0, 30, 33), fw, cw, shard=1)),
                (R.make_shard(rng, rng.randint(-9, 9, 7), fw, cw, shard=0), R.make_shard(rng, rng.randint(-9, 9, 48), fw, cw, shard=1, max_records=40)),
                (R.make_shard(rng, [], fw, cw, shard=0), R.make_shard(rng, [3, 3], fw, cw, shard=1, counts=[2, 5]))]
    _load(a, contents[0][0])
    _load(b, contents[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dst.merge_shards([a, b])                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dst.merge_shards([a, b])
    for sa, sb in contents[1:] + contents[:1]:
        assert sa["n_records"] <= 4096 and sb["n_records"] <= 2048
        _load(a, sa)
        _load(b, sb)
        _poison(dst)
        g.replay()
        torch.cuda.synchronize()
        got = _host(dst)
        eager = _host(_ev(kind, record_capacity=8192).merge_shards([a, b]))
        R.same(got, eager, "replay against eager")
        R.same(got, R.merge([sa, sb], 8192, 256), "replay against the restatement")


# ------------------------------------------------------------------------------------------------------------ 8. image_capacity = 0
@pytest.mark.parametrize("kind", KINDS)
def test_without_a_ledger_nothing_changes(kind):
    frames = _pool(kind)[:12]
    zero, plain = _Feeder(kind, _ev(kind, image_capacity=0)), _Feeder(kind, _ev(kind, image_capacity=None))
    for f in frames:
        zero.feed(f)
        plain.feed(f)
    sz, sp = zero.ev.state(), plain.ev.state()
    want_keys = {"score", "label", "image_id", "flags", "n_records", "error", zero.ev._COLUMN, zero.ev._COUNTER[0]} | set(zero.ev._config())
    assert set(sz) == set(sp) == want_keys and not hasattr(zero.ev, "led_image")
    slot_order = kind == "voc"                                  # the COCO update reserves slots per category workgroup: the order is free there
    for k in sz:
        if not isinstance(sz[k], torch.Tensor):
            assert sz[k] == sp[k], k
        elif slot_order or k not in zero.ev._keys():
            assert _bits(sz[k].cpu().numpy(), sp[k].cpu().numpy()), k
        else:
            assert sz[k].shape == sp[k].shape and sz[k].dtype == sp[k].dtype, k
    ra, rb = zero.ev.records_sorted(), plain.ev.records_sorted()
    for k in ra:
        assert _bits(ra[k], rb[k]), k
    _same_summary(kind, zero.ev.summarize(), plain.ev.summarize())
    other = _Feeder(kind, _ev(kind, image_capacity=0))
    other.feed(_pool(kind)[20])
    n = sz["n_records"]
    zero.ev.merge(other.ev)                                     # the append-only merge as before
    assert zero.ev.state()["n_records"] == n + other.ev.state()["n_records"]
