"""csrc/topk.hip on unlucky samples, special scores and path seams, bit for bit against tests/topk_ref.py.  No tolerance anywhere: the
first count entries of idx, the bit patterns of scores and boxes, and count itself.

  (a) the four "unlucky sample" builders in the default launch form, proposal mode (10 % of the entries -1) and all_live; after each call
      the device's own bucket counts (SsCtl::cnt, 256 int32 at byte 8 * 256 of the workspace the op used) are read back and must equal
      the host mirror's and show what the builder promises: a ranked bucket above 1024 keys, or exactly 1024 and 1025
  (b) the same cases and a random control through each of the three sample-sort launch forms, one fresh child process per form
  (c) every size seam (64 / 256 / 1024 / 4096 / 65536 and their neighbours) with ties on both sides of every border
  (d) +-inf, FLT_MAX, denormals, +-0.0 and NaNs of both signs: the order contract of docs/PARITY.md
  (e) the big-bucket branch between guards, with the exact-size workspace
  (f) the whole proposal stage with the sampling inside the prologue launch
  (g) ops.nms / ops.batched_nms, which visit in the all_live order
tests/test_topk_ref_host.py proves on the CPU that the inputs of (a), (b), (e) and (f) do reach the m > 1024 branch."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guarded as G
import topk_ref as tr
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNT_BYTE = 8 * tr.BUCKETS                     # offsetof(SsCtl, cnt): csrc/frcnn_layout.h asserts it


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


def T(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)         # (topk_ref's cached cases are read-only)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(ops, s, K, boxes=None, all_live=False):
    """(n, idx, scores, boxes) as numpy; s / boxes may be device tensors already"""
    s = s if isinstance(s, torch.Tensor) else T(s)
    boxes = boxes if boxes is None or isinstance(boxes, torch.Tensor) else T(boxes)
    idx, sc, bx, cnt = ops.topk_sorted(s, K, boxes, all_live=all_live)
    return int(cnt.item()), idx.cpu().numpy(), sc.cpu().numpy(), None if bx is None else bx.cpu().numpy()


def same_as_reference(got, ref_idx, s, boxes, what):
    n, idx, sc, bx = got
    assert n == len(ref_idx), (what, "count", n, len(ref_idx))
    bad = np.nonzero(idx[:n] != ref_idx)[0]
    assert len(bad) == 0, (what, "idx differs at rank", int(bad[0]), int(idx[bad[0]]), int(ref_idx[bad[0]]), len(bad))
    assert np.array_equal(bits(sc[:n]), bits(s[ref_idx])), (what, "scores")
    if bx is not None:
        assert np.array_equal(bits(bx[:n]), bits(boxes[ref_idx])), (what, "boxes")


@functools.lru_cache(maxsize=None)
def case_reference(builder, N, K, all_live):
    s, _, K = tr.case_inputs(builder, N, K, all_live)
    return tr.topk(s, K, all_live)[0]


def device_bucket_counts(ops, N):
    """SsCtl::cnt of the last sample sort of N scores on this stream: ops.topk_sorted took its workspace from the same cache"""
    from faster_rcnn_pytorch_amd import _lib
    ws = ops._workspace(torch.device(DEV), _lib.workspace_bytes(_lib.OP_TOPK, N))
    return ws[CNT_BYTE:CNT_BYTE + 4 * tr.BUCKETS].view(torch.int32).cpu().numpy().astype(np.int64)


def buckets_as_promised(builder, N, K, all_live, sizes, n):
    """the device's counts equal the host mirror's, and they show the bucket sizes the builder is there for"""
    s, _, K = tr.case_inputs(builder, N, K, all_live)
    want, _, n_out = tr.bucket_sizes(s, K, all_live)
    assert n == n_out and np.array_equal(sizes, want), (builder, N, K, all_live, "the device counted other buckets than the host mirror")
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    tr.check_promise(builder, N, K, all_live, sizes, first, n)


# ============================================================================================ (a) unlucky samples, default form
@pytest.mark.parametrize("all_live", [False, True], ids=["proposal", "all_live"])
@pytest.mark.parametrize("builder,N,K", tr.UNLUCKY_CASES)
def test_unlucky_samples(ops, builder, N, K, all_live):
    s, boxes, Kc = tr.case_inputs(builder, N, K, all_live)
    got = run(ops, s, Kc, boxes, all_live)
    sizes = device_bucket_counts(ops, N)
    buckets_as_promised(builder, N, K, all_live, sizes, got[0])
    same_as_reference(got, case_reference(builder, N, K, all_live), s, boxes, (builder, N, K, all_live))


# ============================================================================================ (b) every launch form
CHILD = r"""
import json, sys
import numpy as np, torch
from faster_rcnn_pytorch_amd import ops, _lib
d = sys.argv[1]
dev = torch.device("cuda:0")
for c in json.load(open(d + "/cases.json")):
    s = torch.from_numpy(np.load("%s/%s_s.npy" % (d, c["file"]))).to(dev)
    b = torch.from_numpy(np.load("%s/%s_b.npy" % (d, c["file"]))).to(dev)
    idx, sc, bx, cnt = ops.topk_sorted(s, c["K"], b, all_live=c["all_live"])
    n = int(cnt.item())
    ws = ops._workspace(dev, _lib.workspace_bytes(_lib.OP_TOPK, c["N"]))
    np.savez("%s/%s_out.npz" % (sys.argv[2], c["file"]), n=n, idx=idx[:max(n, 0)].cpu().numpy(), sc=sc[:max(n, 0)].cpu().numpy(),
             bx=bx[:max(n, 0)].cpu().numpy(), cnt=ws[2048:3072].view(torch.int32).cpu().numpy())
torch.cuda.synchronize()
"""


def _form_cases():
    return [(b, n, k, al) for b, n, k in tr.UNLUCKY_CASES + (tr.RANDOM_CASE,) for al in (False, True)]


@pytest.fixture(scope="module")
def form_inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("topk_forms"))
    manifest = []
    for i, (b, n, k, al) in enumerate(_form_cases()):
        s, boxes, kc = tr.case_inputs(b, n, k, al)
        np.save(os.path.join(d, "%d_s.npy" % i), s)
        np.save(os.path.join(d, "%d_b.npy" % i), boxes)
        manifest.append({"file": str(i), "N": n, "K": kc, "all_live": al})
    with open(os.path.join(d, "cases.json"), "w") as f:
        json.dump(manifest, f)
    return d


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_unlucky_samples_in_every_launch_form(form_inputs, tmp_path, fused):
    """FRCNN_TOPK_FUSED is read once per process: 0 = count / place / bucket launches, 1 = partition + bucket, 2 = one launch, whose
    ranking phase holds the second copy of the m > 1024 branch (agent-scope loads behind the grid barrier).  The defaults never run
    form 2 below N = 65536 nor form 1 from there on."""
    env = dict(os.environ, PYTHONPATH=ROOT, FRCNN_TOPK_FUSED=str(fused))
    subprocess.run([sys.executable, "-c", CHILD, form_inputs, str(tmp_path)], check=True, env=env, timeout=300)
    for i, (b, n, k, al) in enumerate(_form_cases()):
        s, boxes, _ = tr.case_inputs(b, n, k, al)
        out = np.load(os.path.join(str(tmp_path), "%d_out.npz" % i))
        got = (int(out["n"]), out["idx"], out["sc"], out["bx"])
        buckets_as_promised(b, n, k, al, out["cnt"].astype(np.int64), got[0])
        same_as_reference(got, case_reference(b, n, k, al), s, boxes, ("FRCNN_TOPK_FUSED=%d" % fused, b, n, k, al))


# ============================================================================================ (c) size seams with ties
@pytest.mark.parametrize("N", tr.SEAM_N)
def test_size_seams_with_ties(ops, N):
    """4095 / 4096: rank sort -> sample sort; 65535 / 65536: 512 -> 2048 samples, 4 -> 8 parts per bucket, two launches -> one; multiples
    of the 64-column chunk, the 256-row block and the 1024-column segment of the rank sort, each with its two neighbours."""
    boxes = tr.rand_boxes(np.random.RandomState(N), N)
    tb = T(boxes)
    dead = tr.seam_dead(N)
    for kind in tr.SEAM_INPUTS:
        s = tr.seam_scores(kind, N)
        ts = T(s)
        full = tr.topk(s, N, all_live=True)[0]
        for b in (tb, None):
            same_as_reference(run(ops, ts, N, b, True), full, s, boxes, (kind, N, "all_live", b is not None))
        sd = s.copy()
        sd[dead] = -1.0
        tsd = T(sd)
        live, n_live = tr.topk(sd, N)
        for K in sorted({K for K in (1, n_live - 1, n_live, n_live + 1, N) if 1 <= K <= N}):
            for b in (tb, None):
                same_as_reference(run(ops, tsd, K, b), live[:K], sd, boxes, (kind, N, K, b is not None))


# ============================================================================================ (d) special scores
SPECIAL_N = (300, 3000, 5000)                 # one segment of the rank sort; three segments and twelve row blocks; the sample sort


@pytest.mark.parametrize("with_nan", [False, True], ids=["finite_inf_zero", "nan"])
@pytest.mark.parametrize("N", SPECIAL_N)
def test_special_scores_follow_the_order_contract(ops, N, with_nan):
    s = tr.special_scores(N, with_nan)
    boxes = tr.rand_boxes(np.random.RandomState(N), N)
    # every entry live: the total order on the bit patterns (-0.0 after +0.0, sign-clear NaNs first, sign-set NaNs last)
    ref, _ = tr.topk(s, N, all_live=True)
    k = tr.key32(s[ref]).astype(np.int64)
    assert (np.diff(k) <= 0).all() and (np.diff(ref)[np.diff(k) == 0] > 0).all()
    same_as_reference(run(ops, s, N, boxes, True), ref, s, boxes, (N, "all_live"))
    # proposal mode: score >= 0 is live -- -0.0 and the denormals are, a negative denormal and every NaN are not
    n_live = int(tr.live_mask(s).sum())
    for K in (N, n_live, N // 3):
        ref, n = tr.topk(s, K)
        assert n == min(K, n_live) and not np.isnan(s[ref]).any() and (s[ref] >= 0).all()
        got = run(ops, s, K, boxes)
        assert got[0] == min(K, n_live), (N, K, "count", got[0], min(K, n_live))
        assert not np.isnan(got[2][:got[0]]).any(), (N, K, "a NaN row was emitted")
        same_as_reference(got, ref, s, boxes, (N, K, "proposal"))                           # no live row displaced


@pytest.mark.parametrize("N", SPECIAL_N)
def test_nan_scores_in_proposal_mode_leave_no_element_unwritten(ops, N):
    """Under 0xFF and under 0x00 fills: the outputs below count are the same bytes, so every one of them was written by the kernels (a
    sign-clear NaN that out-ranks the live scores without being live left out_idx[0 .. nNaN - 1] as the allocator handed it over)."""
    s = tr.special_scores(N, True)
    boxes = tr.rand_boxes(np.random.RandomState(N), N)

    def case(g):
        idx, sc, bx, cnt = ops.topk_sorted(g.place(T(s)), N, g.place(T(boxes)))
        m = int(cnt.item())
        return {"count": cnt, "idx": idx[:m], "scores": sc[:m], "boxes": bx[:m]}
    out = G.run_both(case)[0]
    ref, n = tr.topk(s, N)
    got = (int(out["count"].item()), out["idx"].cpu().numpy(), out["scores"].cpu().numpy(), out["boxes"].cpu().numpy())
    same_as_reference(got, ref, s, boxes, (N, "guarded"))


# ============================================================================================ (e) guards on the branch
@pytest.mark.parametrize("all_live", [False, True], ids=["proposal", "all_live"])
@pytest.mark.parametrize("builder,N,K", [("low_samples", 20646, 12000), ("exact_1024_1025", 8192, 8192)])
def test_big_bucket_branch_between_guards(ops, builder, N, K, all_live):
    """Every operand, output and the workspace -- at exactly frcnn_ws_topk(N) bytes -- between two poisoned guards: the row groups x
    1024-key chunks of the big-bucket branch touch nothing outside them, and the outputs below count do not depend on the fill."""
    s, boxes, Kc = tr.case_inputs(builder, N, K, all_live)

    def case(g):
        idx, sc, bx, cnt = ops.topk_sorted(g.place(T(s)), Kc, g.place(T(boxes)), all_live=all_live)
        m = int(cnt.item())
        return {"count": cnt, "idx": idx[:m], "scores": sc[:m], "boxes": bx[:m]}
    out = G.run_both(case)[0]
    got = (int(out["count"].item()), out["idx"].cpu().numpy(), out["scores"].cpu().numpy(), out["boxes"].cpu().numpy())
    same_as_reference(got, case_reference(builder, N, K, all_live), s, boxes, (builder, N, K, all_live))


# ============================================================================================ (f) whole proposal stage
@pytest.mark.parametrize("K,P", [(12000, 2000), (6000, 300)])
@pytest.mark.parametrize("which", ["low", "high"])
def test_region_proposal_with_an_unlucky_sample_in_the_prologue(ops, which, K, P):
    """600 x 1000: the splitters are drawn inside the prologue launch (ss_sample_body on prologue_one's scores) from anchors whose
    objectness is the lowest / the highest of the map, so the ranking that follows meets one bucket of more than 15 000 keys."""
    H, W = 600, 1000
    anchor = orc.anchor_grid(H, W)
    reg, cls = tr.proposal_logits(len(anchor), K, which)
    rois_o, src_o = orc.region_proposal(reg, cls, anchor, 1 / 1000, K, 0.7, P)
    grid = (H // 16, W // 16, 16, ops.anchor_base(), W, H)
    for anchors, g in ((T(anchor), None), (None, grid)):                                    # anchors from HBM / regenerated in registers
        rois, cnt, src = ops.region_proposal(T(reg), T(cls), anchors, 1 / 1000, K, 0.7, P, grid=g, want_src=True)
        n = int(cnt.item())
        assert n == len(rois_o), (which, K, P, g is not None, n, len(rois_o))
        assert np.array_equal(src[:n].cpu().numpy(), src_o) and np.array_equal(bits(rois[:n].cpu().numpy()), bits(rois_o))


# ============================================================================================ (g) the drop-ins
@pytest.mark.parametrize("N", [4500, 70])
def test_nms_drop_ins_visit_in_the_all_live_order(ops, N):
    """Heavy ties, negatives and -0.0: ops.nms / ops.batched_nms visit the boxes in topk_ref's all_live order (4500: sample sort, 70: rank
    sort), per class for the batched form."""
    rng = np.random.RandomState(N)
    pool = np.array([-0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 0.75], np.float32)
    s = pool[rng.randint(0, len(pool), N)]
    b = tr.rand_boxes(rng, N, 0.05, 0.4)
    cl = rng.randint(0, 4, N).astype(np.int64)
    order, _ = tr.topk(s, N, all_live=True)
    assert np.array_equal(ops.nms(T(b), T(s), 0.5).cpu().numpy(), orc.nms(b, 0.5, order=order))
    rank = np.empty(N, np.int64)
    rank[order] = np.arange(N)
    members = [np.nonzero(cl == q)[0] for q in range(4)]                                     # ascending: a class keeps the global tie-break
    exp = np.concatenate([m[orc.nms(b[m], 0.5, order=tr.topk(s[m], len(m), all_live=True)[0])] for m in members])
    exp = exp[np.argsort(rank[exp])]
    assert np.array_equal(ops.batched_nms(T(b), T(s), T(cl), 0.5).cpu().numpy(), exp)
