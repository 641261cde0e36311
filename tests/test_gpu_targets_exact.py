"""The RPN and head target makers (csrc/targets.hip) on EXACT data at their seams, against tests/targets_ref.py: an independent
restatement in integers and rationals that tests/test_targets_ref_host.py has tied to the C oracle on the CPU and whose guard
guarantees that fp32 cannot merge or reorder any comparison of a case.

Checked for every case: labels, counts, kept rows, classes and sampled RoIs bit for bit; regression targets columns 0-1 bit for bit
against the fp32 rounding of the exact rational (a lattice subtraction and correctly rounded divisions); columns 2-3 against
float64 log within the suite's bounds (RPN 1e-6, head 1e-5 after the / 0.2).

Forms: every RPN case runs with host permutations (rpn_colmax -> rpn_label -> rpn_sample), in device-RNG mode (the fused
rpn_match_kernel, inline or with rpn_apply_kernel; expected labels = the restatement fed the Philox permutations) and once more in ONE
child process with FRCNN_RPN_FUSED=0 (rpn_colmax -> rpn_label<KEYS> -> rpn_apply).  Every head case runs with host permutations and
in device-RNG mode."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import targets_ref as tr
from oracle import philox_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RPN_NAMES = tr.rpn_case_names()
HEAD_NAMES = tr.head_case_names()
SEED, OFFSET = (3 << 32) | 17, (1 << 32) | 5          # both halves of both words in use


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_log_columns(got, want, tol, what):
    """finite targets within tol of float64 log; a zero divisor's +-inf / nan identical"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    if fin.any():
        err = np.abs(got[fin] - want[fin]).max()
        print("%s: log columns max |err| = %.3g (bound %g)" % (what, err, tol))
        assert err < tol, what


def _check_rpn(c, cls, reg, counts, want_labels, what):
    r = tr.rpn_match(c)
    what = "%s [%s]" % (c.name, what)
    assert list(counts[:3]) == [r.n_pos, r.n_neg, 0], what
    bad = np.nonzero(np.asarray(cls) != want_labels)[0]
    assert bad.size == 0, "%s: %d labels differ, first at anchor %d: got %d, want %d" % (what, bad.size, bad[0], cls[bad[0]], want_labels[bad[0]])
    assert np.array_equal(_bits(reg[:, :2]), _bits(r.reg01)), what
    _check_log_columns(reg[:, 2:], r.reg23, 1e-6, what)


def _host_perms(c):
    """both permutations, always (a missing pair would select device-RNG mode); the reference's draw where it draws one"""
    r = tr.rpn_match(c)
    pp, pn = tr.rpn_perms(c)
    return (np.arange(r.n_pos) if pp is None else pp), (np.arange(r.n_neg) if pn is None else pn)


def _philox_labels(c, seed, offset):
    r = tr.rpn_match(c)
    pp = philox_ref.sampling_perm(seed, offset, 1, np.nonzero(r.pre == 1)[0])
    pn = philox_ref.sampling_perm(seed, offset, 0, np.nonzero(r.pre == 0)[0])
    return tr.rpn_sample(c, pp, pn)


# ------------------------------------------------------------------------------------------------ RPN
@pytest.mark.parametrize("name", RPN_NAMES)
def test_rpn_exact_case_with_host_permutations(ops, name):
    c = tr.rpn_case(name)
    tr.check_decidable(c)
    pp, pn = _host_perms(c)
    cls, reg, counts = ops.rpn_targets(T(tr.to_f32(c.anchors)), T(tr.to_f32(c.gt)), variant=c.variant, perm_pos=pp, perm_neg=pn)
    _check_rpn(c, cls.cpu().numpy(), reg.cpu().numpy(), counts.cpu().tolist(), tr.rpn_sample(c, pp, pn), "host permutations")


@pytest.mark.parametrize("name", RPN_NAMES)
def test_rpn_exact_case_in_device_rng_mode(ops, name):
    c = tr.rpn_case(name)
    tr.check_decidable(c)
    cls, reg, counts = ops.rpn_targets(T(tr.to_f32(c.anchors)), T(tr.to_f32(c.gt)), variant=c.variant, seed=SEED, offset=OFFSET)
    _check_rpn(c, cls.cpu().numpy(), reg.cpu().numpy(), counts.cpu().tolist(), _philox_labels(c, SEED, OFFSET), "device RNG, fused")


_CHILD = ("import numpy as np, torch, sys; from faster_rcnn_pytorch_amd import ops; d = sys.argv[1]\n"
          "z = np.load(d + '/in.npz'); out = {}\n"
          "for k in range(int(z['n'])):\n"
          "    r = ops.rpn_targets(torch.from_numpy(z['a%d' % k]).cuda(), torch.from_numpy(z['g%d' % k]).cuda(), variant=int(z['v'][k]), seed=int(sys.argv[2]), offset=int(sys.argv[3]))\n"
          "    out['cls%d' % k], out['reg%d' % k], out['cnt%d' % k] = (x.cpu().numpy() for x in r)\n"
          "np.savez(d + '/out.npz', **out)\n")


@pytest.fixture(scope="module")
def staged_child():
    """every RPN case through the staged device-RNG form: ONE fresh child process with FRCNN_RPN_FUSED=0"""
    cases = [tr.rpn_case(n) for n in RPN_NAMES]
    arrays = {"n": np.int64(len(cases)), "v": np.array([c.variant for c in cases], np.int64)}
    for k, c in enumerate(cases):
        arrays["a%d" % k], arrays["g%d" % k] = tr.to_f32(c.anchors), tr.to_f32(c.gt)
    with tempfile.TemporaryDirectory() as d:
        np.savez(os.path.join(d, "in.npz"), **arrays)
        env = dict(os.environ, FRCNN_RPN_FUSED="0", PYTHONPATH=ROOT)
        subprocess.run([sys.executable, "-c", _CHILD, d, str(SEED), str(OFFSET)], check=True, env=env, timeout=300)
        z = np.load(os.path.join(d, "out.npz"))
        return {c.name: (z["cls%d" % k], z["reg%d" % k], z["cnt%d" % k]) for k, c in enumerate(cases)}


@pytest.mark.parametrize("name", RPN_NAMES)
def test_rpn_exact_case_in_staged_device_rng_form(staged_child, name):
    c = tr.rpn_case(name)
    cls, reg, counts = staged_child[name]
    _check_rpn(c, cls, reg, counts.tolist(), _philox_labels(c, SEED, OFFSET), "device RNG, staged child")


def test_rpn_inline_bound_24576_is_one_launch_and_24577_two(ops):
    from faster_rcnn_pytorch_amd import _lib
    seen = {}
    _lib.prof_enable(True)
    try:
        for N in (24576, 24577):
            c = tr.rpn_case("N%d-v0" % N)
            a, g = T(tr.to_f32(c.anchors)), T(tr.to_f32(c.gt))
            _lib.prof_reset()
            ops.rpn_targets(a, g, variant=0, seed=1, offset=2)
            seen[N] = {k: v[1] for k, v in _lib.prof_report().items()}
    finally:
        _lib.prof_enable(False)
    assert seen[24576] == {"rpn_match_kernel": 1}, seen
    assert seen[24577] == {"rpn_match_kernel": 1, "rpn_apply_kernel": 1}, seen


def test_rpn_4097_gts_are_refused_not_launched(ops):
    from faster_rcnn_pytorch_amd import _lib
    a = T(tr.to_f32([tr.slot_gt(0)] * 8))                   # exact copies: IoU >= 0.7 with every gt
    g = T(tr.to_f32([tr.slot_gt(0)] * 4097))
    for kw in (dict(seed=1), dict(perm_pos=np.arange(8), perm_neg=np.arange(8))):
        with pytest.raises(_lib.FrcnnError, match="above limit 4096"):
            ops.rpn_targets(a, g, **kw)
    cls = ops.rpn_targets(a, g[:4096], seed=1)[0]              # the limit itself is served
    assert cls.cpu().tolist() == [1] * 8


# ------------------------------------------------------------------------------------------------ head
def _check_head(c, out, pp, pn, what):
    cls, reg, srois, keep, counts = (x.cpu().numpy() for x in out)
    r = tr.head_match(c)
    what = "%s [%s]" % (c.name, what)
    keep_w, cls_w, reg01_w, reg23_w, counts_w = tr.head_sample(c, pp, pn)
    rows = counts_w[2]
    assert counts.tolist() == counts_w, what
    assert np.array_equal(keep[:rows], keep_w), what
    assert np.array_equal(cls[:rows], cls_w), what
    assert np.array_equal(_bits(srois[:rows]), _bits(tr.to_f32(r.cand[keep_w]))), what
    assert np.array_equal(_bits(reg[:rows, :2]), _bits(reg01_w)), what
    _check_log_columns(reg[:rows, 2:], reg23_w, 1e-5, what)
    # rows that could not be sampled: class -1, no candidate, zeros
    assert (cls[rows:] == -1).all() and (keep[rows:] == -1).all() and not srois[rows:].any() and not reg[rows:].any(), what


def _head_call(ops, c, **kw):
    n_rois = T(np.array([c.n_rois], np.int32)) if c.n_rois != c.rois.shape[0] else None
    return ops.head_targets(T(c.rois_f32()), T(tr.to_f32(c.gt)), T(c.gt_label), n_rois=n_rois, variant=c.variant, label_offset=c.label_offset,
                            max_pos=c.max_pos, total=c.total, want_keep=True, **kw)


@pytest.mark.parametrize("name", HEAD_NAMES)
def test_head_exact_case_with_host_permutations(ops, name):
    c = tr.head_case(name)
    tr.check_decidable(c)
    for kind in ("identity", "reversed", "random"):
        pp, pn = tr.head_perms(c, kind)
        _check_head(c, _head_call(ops, c, perm_pos=pp, perm_neg=pn), pp, pn, kind + " permutations")
        if kind == "identity":                                   # the kept list is the candidates in ascending order across the rounds
            keep = tr.head_sample(c, pp, pn)[0]
            n_pos = min(tr.head_match(c).npc, c.max_pos)
            assert (np.diff(keep[:n_pos]) > 0).all() and (np.diff(keep[n_pos:]) > 0).all()


@pytest.mark.parametrize("name", HEAD_NAMES)
def test_head_exact_case_in_device_rng_mode(ops, name):
    c = tr.head_case(name)
    tr.check_decidable(c)
    r = tr.head_match(c)
    pp = philox_ref.sampling_perm(SEED, OFFSET, 2, r.pos_list)
    pn = philox_ref.sampling_perm(SEED, OFFSET, 3, r.neg_list)
    _check_head(c, _head_call(ops, c, seed=SEED, offset=OFFSET), pp, pn, "device RNG")


def test_head_limits_are_refused_not_launched(ops):
    from faster_rcnn_pytorch_amd import _lib
    gt, lab = T(tr.to_f32(tr.HEAD_GT)), T(np.asarray(tr.HEAD_LAB, np.int64))
    rois = T(tr.to_f32([tr._neg_box(k) for k in range(4094)]))
    with pytest.raises(_lib.FrcnnError, match="above limit 4096"):            # P_cap + G = 4097, whatever the device count says
        ops.head_targets(rois, gt, lab, n_rois=T(np.array([10], np.int32)), seed=1)
    with pytest.raises(_lib.FrcnnError, match="total"):
        ops.head_targets(rois[:2000], gt, lab, max_pos=32, total=1025, seed=1)
    counts = ops.head_targets(rois[:4093], gt, lab, seed=1)[4]              # 4096 candidates are served
    assert counts.cpu().tolist() == [3, 4093, 128, 0]
