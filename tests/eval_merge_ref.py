"""The merge of evaluator shards (csrc/eval_merge.hip, evaluation._RecordStore.merge_shards) restated with numpy, and the synthetic
shards the tests feed it.

A shard is a dict of host arrays, the live part of an evaluator's state(): the record columns score f32, label / image_id / order i32 [n],
flags i32 [n] or [n, 4]; the ledger led_image i32 [m], led_range i64 [m, 2] (the record slots [begin, end) of every frame, ascending),
led_delta i32 [m, CW]; n_records, n_images (what the shard counted) and error.

Semantics (the reference's merge, evaluation/coco_eval.py:161-180, pinned by tests/test_eval_merge_host.py to tests/golden/eval_merge.npz):
occurrences are ordered (shard, ledger row); an occurrence is kept iff no earlier occurrence has its image_id."""
import numpy as np

COLUMNS = ("score", "label", "image_id", "order", "flags")
ERR_LEDGER_OVERFLOW, ERR_SHARD_TRUNCATED = 16, 32


def kept_occurrences(ids_per_shard):
    """[(shard, row)] of the kept occurrences, in (shard, row) order."""
    seen, kept = set(), []
    for w, ids in enumerate(ids_per_shard):
        for r, v in enumerate(ids):
            if int(v) not in seen:
                seen.add(int(v))
                kept.append((w, r))
    return kept


def merge(shards, record_capacity=None, image_capacity=None):
    """The merged store as a shard dict plus "counter" i64 [CW]: the records of kept occurrences in (shard, slot) order, their ledger rows
    with rebased ranges, the sum of their deltas.  n_records / n_images count everything kept; the arrays are cut at the capacities."""
    cw = shards[0]["led_delta"].shape[1]
    out = {k: [] for k in COLUMNS}
    led_image, led_range, led_delta = [], [], []
    counter, n, err = np.zeros(cw, np.int64), 0, 0
    for w, r in kept_occurrences([s["led_image"][:min(int(s["n_images"]), len(s["led_image"]))] for s in shards]):
        s = shards[w]
        live = min(int(s["n_records"]), len(s["score"]))
        b = min(max(int(s["led_range"][r, 0]), 0), live)
        e = min(max(int(s["led_range"][r, 1]), b), live)
        for k in COLUMNS:
            out[k].append(s[k][b:e])
        led_image.append(s["led_image"][r])
        led_range.append((n, n + e - b))
        led_delta.append(s["led_delta"][r])
        counter += s["led_delta"][r].astype(np.int64)
        n += e - b
    for s in shards:
        err |= int(s["error"])
        if int(s["n_records"]) > len(s["score"]) or int(s["n_images"]) > len(s["led_image"]):
            err |= ERR_SHARD_TRUNCATED
    m = len(led_image)
    if image_capacity is not None and m > image_capacity:
        err |= ERR_LEDGER_OVERFLOW
    res = {k: (np.concatenate(out[k]) if out[k] else shards[0][k][:0])[:record_capacity] for k in COLUMNS}
    res.update(led_image=np.array(led_image, np.int32)[:image_capacity], led_range=np.array(led_range, np.int64).reshape(-1, 2)[:image_capacity],
               led_delta=np.array(led_delta, np.int32).reshape(-1, cw)[:image_capacity], counter=counter, n_records=n, n_images=m, error=err)
    return res


def same(a, b, what=""):
    """a and b agree bit for bit in every column, the ledger, the counts, the error word and (where both have one) the counter."""
    for k in ("n_records", "n_images", "error"):
        assert int(a[k]) == int(b[k]), (what, k, int(a[k]), int(b[k]))
    for k in COLUMNS + ("led_image", "led_range", "led_delta") + (("counter",) if "counter" in a and "counter" in b else ()):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype.itemsize == y.dtype.itemsize, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


def make_shard(rng, ids, flags_width=1, counter_words=5, max_records=6, shard=0, counts=None):
    """A consistent shard over the frames `ids`: frame r owns counts[r] (default: 0 .. max_records at random, every third frame none)
    consecutive records, whose score encodes (shard, row, position) so that a wrong selection shows; the scores also hold -0.0, NaN
    payloads and denormals, which must travel bit for bit."""
    m = len(ids)
    if counts is None:
        counts = [0 if r % 3 == 2 else int(rng.randint(0, max_records + 1)) for r in range(m)]
    ends = np.cumsum([0] + list(counts)).astype(np.int64)
    n = int(ends[-1])
    score = (shard * 4096.0 + np.repeat(np.arange(m), counts) + rng.randint(0, 8, n) / 8.0).astype(np.float32)
    odd = np.array([0x80000000, 0x7FC00001, 0xFFC12345, 0x00000001, 0x7F800000], np.uint32).view(np.float32)
    for i in range(0, n, 7):
        score[i] = odd[(i // 7) % len(odd)]
    fl = rng.randint(0, 1 << 31, (n, flags_width)).astype(np.int32)
    return {"score": score, "label": rng.randint(0, 5, n).astype(np.int32), "image_id": np.repeat(np.asarray(ids, np.int32), counts).astype(np.int32),
            "order": np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32),
            "flags": fl[:, 0] if flags_width == 1 else fl, "led_image": np.asarray(ids, np.int32).reshape(m),
            "led_range": np.stack([ends[:-1], ends[1:]], 1).astype(np.int64).reshape(m, 2),
            "led_delta": rng.randint(-2, 9, (m, counter_words)).astype(np.int32), "n_records": n, "n_images": m, "error": 0}


def golden_cases(z):
    """{name: (ids per shard, merged ids, selected (shard, row))} of tests/golden/eval_merge.npz."""
    out = {}
    for name in z["cases"].tolist():
        ids, off = z[name + "__ids"], z[name + "__offsets"]
        out[name] = ([ids[off[w]:off[w + 1]] for w in range(len(off) - 1)], z[name + "__merged_ids"], z[name + "__selected"])
    return out
