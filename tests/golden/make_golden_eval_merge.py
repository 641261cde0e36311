"""Generates tests/golden/eval_merge.npz by RUNNING the reference's own merge (evaluation/coco_eval.py:161-180 merge(img_ids, eval_imgs):
all_gather, concatenate, np.unique(..., return_index=True)) on synthetic id lists.  The module is loaded by file path with pycocotools,
torchvision and util.misc stubbed (none of them is touched by merge), and util.misc.all_gather replaced by a function that returns the
prepared list of shards.  The cells of eval_imgs encode (shard, row), so what comes back says which occurrence of every image id the
reference keeps.  Only inputs and results are stored: per case the ids of all shards, the shard offsets, the merged ids and the selected
(shard, row) pairs, and the counts of the kinds the set is asserted to contain.  Re-run:  python tests/golden/make_golden_eval_merge.py"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get("FRCNN_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
I32 = np.iinfo(np.int32)


def load_reference(gathered):
    """evaluation/coco_eval.py with its imports stubbed; all_gather hands out gathered.pop(0)."""
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    for name, attrs in (("pycocotools", {}), ("pycocotools.cocoeval", {"COCOeval": object}), ("pycocotools.coco", {"COCO": object}),
                        ("pycocotools.mask", {}), ("util", {}), ("util.misc", {"all_gather": lambda _: gathered.pop(0)})):
        stub(name, **attrs)
    try:
        import torchvision  # noqa: F401
    except Exception:                                           # noqa: BLE001
        stub("torchvision")
    spec = importlib.util.spec_from_file_location("ref_coco_eval", os.path.join(REF, "evaluation", "coco_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sampler_shards(ids, W):
    """torch.utils.data.DistributedSampler(shuffle=False, drop_last=False): the index list padded with its own head to a multiple of W,
    rank r takes every W-th index from r."""
    idx = list(range(len(ids)))
    total = -(-len(idx) // W) * W
    idx += idx[:total - len(idx)]
    return [[ids[i] for i in idx[r::W]] for r in range(W)]


def cases():
    rng = np.random.RandomState(161)
    c = {}
    for W, n in ((2, 11), (3, 20), (8, 37)):
        c["sampler_w%d" % W] = sampler_shards([int(v) for v in 1000 + 7 * rng.permutation(n)], W)
    c["dup_inside_shard"] = [[5, 9, 5, 3, 9], [3, 12, 12]]
    c["empty_shard"] = [[4, 2], [], [2, 8, 4]]
    c["empty_first_shard"] = [[], [6, 6, 1]]
    c["single_shard"] = [[7, 3, 7, 1, 3, 3]]
    c["all_identical"] = [[10, 11, 12, 13]] * 4
    c["extreme_ids"] = [[0, -1, int(I32.min), int(I32.max)], [int(I32.min), -1, -2, 0], [int(I32.max), 1, -1]]
    c["random_w5"] = [[int(v) for v in rng.randint(-20, 20, rng.randint(0, 30))] for _ in range(5)]
    return c


def kinds(c):
    k = dict.fromkeys(["sampler_padding_w2", "sampler_padding_w3", "sampler_padding_w8", "duplicate_inside_one_shard", "empty_shard", "single_shard",
                       "all_shards_identical", "negative_ids", "extreme_ids"], 0)
    for name, shards in c.items():
        flat = [v for s in shards for v in s]
        W = len(shards)
        if name.startswith("sampler") and len(flat) > len(set(flat)) and len(set(len(s) for s in shards)) == 1:
            k["sampler_padding_w%d" % W] += shards[-1][-1] in [s[0] for s in shards[:-1]]      # the ids wrap round to the first images
        k["duplicate_inside_one_shard"] += any(len(s) > len(set(s)) for s in shards)
        k["empty_shard"] += any(len(s) == 0 for s in shards)
        k["single_shard"] += W == 1
        k["all_shards_identical"] += W > 1 and all(s == shards[0] for s in shards) and len(shards[0]) > 0
        k["negative_ids"] += any(v < 0 for v in flat)
        k["extreme_ids"] += int(I32.min) in flat and int(I32.max) in flat and 0 in flat and -1 in flat
    return {a: int(b) for a, b in k.items()}


def main():
    gathered = []
    ref = load_reference(gathered)
    c = cases()
    counts = kinds(c)
    for a, b in counts.items():
        assert b >= 1, "the golden set lacks the kind '%s'" % a
    d = {"cases": np.array(sorted(c)), "kinds": np.array(sorted(counts)), "kind_counts": np.array([counts[a] for a in sorted(counts)], np.int64)}
    for name in sorted(c):
        shards = c[name]
        cells = []
        for w, s in enumerate(shards):                          # eval_imgs [K, A, I]: cell (0, 0) = shard, cell (0, 1) = row
            e = np.zeros((1, 2, len(s)), np.int64)
            e[0, 0], e[0, 1] = w, np.arange(len(s))
            cells.append(e)
        gathered[:] = [[list(s) for s in shards], cells]
        ids, imgs = ref.merge(list(shards[0]), cells[0])        # the arguments only feed all_gather
        d[name + "__ids"] = np.array([v for s in shards for v in s], np.int64).astype(np.int32)
        d[name + "__offsets"] = np.cumsum([0] + [len(s) for s in shards]).astype(np.int64)
        d[name + "__merged_ids"] = np.asarray(ids, np.int64).astype(np.int32)
        d[name + "__selected"] = np.stack([imgs[0, 0], imgs[0, 1]], 1).astype(np.int64)
    np.savez_compressed(os.path.join(OUT, "eval_merge.npz"), **d)
    print("eval_merge.npz: %d cases; kinds: %s" % (len(c), counts))


if __name__ == "__main__":
    main()
