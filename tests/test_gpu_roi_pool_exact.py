"""RoIPool on every launch path and at its geometric seams, bit for bit against tests/roi_pool_ref.py (proved on the CPU by
tests/test_roi_pool_ref_host.py: the reference equals the C oracle in every bit on every case here, and every census a case claims holds).

Every case goes through the C ABI in both argmax widths (frcnn_roi_pool_fwd / _bwd with int32, frcnn_roi_pool_fwd_a16 / _bwd_a16 with
uint16, 0xFFFF = -1), each call inside guarded.run_both: once over 0xFF bytes and once over 0x00, so an element of out, argmax or grad_feat
that is not written (an empty bin, a pixel no RoI reaches, a plane behind the global-atomic form's memset) differs between the two runs, and
a byte written outside the outputs trips a guard.  Forward values are compared on their bit patterns (-0.0 is not 0.0) and the argmax
exactly; the backward runs on integer dOut in [-8, 8] with |sum| < 2^24 (asserted by the reference), where every order of additions is
exact: the expectation is float32(ref64) in every bit, no tolerance.  Each case first asserts through ops.roi_pool_plan that it takes the
path its name claims.

Which case names which form (every form frcnn_roi_pool_plan can return):
    forward  lds            geometry / values / launch / rank cases, planes up to 48 x 64       generic        5 x 5 bins; planes from 7 x 439
    backward private8       even-C 16-bit cases up to plane:32x79 (exactly 163 840 B), rank 24 x 24
             private4       plane:3x843, 48x64, 48x106 (exactly 163 840 B), rank 24 x 106
             shared_cb      odd C, 16-bit plane:7x727 and 64x128 (65 536 B); int32 up to 64 x 128; FRCNN_ROI_BWD_SHARED in a child process
             one_channel    int32 plane:3x2731, 128x128 (65 536 B)           global_atomic  int32 plane:5x3277
Run on the GPU box:  python -m pytest tests/test_gpu_roi_pool_exact.py -m gpu -s
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import guarded
import roi_pool_ref as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


def L():
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def N16(t):
    """uint16 device tensor -> int32 numpy argmax (-1 = 0xFFFF)"""
    a = t.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int32)
    return np.where(a == 0xFFFF, -1, a)


def stream():
    return torch.cuda.current_stream().cuda_stream


def assert_same(name, what, got, want):
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s %s: %d of %d values differ, first at %s: %r vs %r" % (
        name, what, bad.sum(), bad.size, np.argwhere(bad)[0], np.asarray(got)[tuple(np.argwhere(bad)[0])], np.asarray(want)[tuple(np.argwhere(bad)[0])])


# ---------------------------------------------------------------------------------------------- the four entry points under guards
def forward(c, P, wide):
    """wide: int32 argmax (frcnn_roi_pool_fwd, P x P bins) or the 16-bit pair.  -> (out numpy, argmax int32 numpy, argmax device tensor)"""
    lib, check = L().lib, L().check

    def case(g):
        feat, rois = g.place(T(c.feat)), g.place(T(c.rois))
        out = torch.empty((c.R, c.C, P, P), dtype=torch.float32, device=DEV)
        arg = torch.empty((c.R, c.C, P, P), dtype=torch.int32 if wide else torch.uint16, device=DEV)
        if wide:
            check(lib.frcnn_roi_pool_fwd(feat.data_ptr(), c.C, c.H, c.W, rois.data_ptr(), c.R, P, P, c.scale, out.data_ptr(), arg.data_ptr(), stream()), "roi_pool_fwd")
        else:
            check(lib.frcnn_roi_pool_fwd_a16(feat.data_ptr(), c.C, c.H, c.W, rois.data_ptr(), c.R, c.scale, out.data_ptr(), arg.data_ptr(), stream()), "roi_pool_fwd_a16")
        return {"out": out, "argmax": arg}
    res, _ = guarded.run_both(case)
    arg = res["argmax"]
    return res["out"].cpu().numpy(), (arg.cpu().numpy() if wide else N16(arg)), arg


def backward(c, P, wide, go, arg_dev, with_rois=True):
    """-> grad_feat numpy [C, H, W]; arg_dev: int32 (wide) or uint16 device tensor"""
    lib, check = L().lib, L().check

    def case(g):
        g_o, arg = g.place(T(go)), g.place(arg_dev)
        rois = g.place(T(c.rois)) if with_rois and not wide else None
        gf = torch.empty((c.C, c.H, c.W), dtype=torch.float32, device=DEV)
        if wide:
            check(lib.frcnn_roi_pool_bwd(g_o.data_ptr(), arg.data_ptr(), c.R, c.C, c.H, c.W, P, P, gf.data_ptr(), stream()), "roi_pool_bwd")
        else:
            check(lib.frcnn_roi_pool_bwd_a16(g_o.data_ptr(), arg.data_ptr(), None if rois is None else rois.data_ptr(), c.scale, c.R, c.C, c.H, c.W,
                                             gf.data_ptr(), stream()), "roi_pool_bwd_a16")
        return {"grad_feat": gf}
    res, _ = guarded.run_both(case)
    return res["grad_feat"].cpu().numpy()


def arg16_dev(arg):
    return T(rp.a16(arg).view(np.int16)).view(torch.uint16)


def check_pair(ops, name, P, wide, fwd_form, bwd_form, fwd_runs=True):
    """forward + backward of one entry-point pair against the reference, after the plan says which kernels these are"""
    c = rp.case(name)
    plan = ops.roi_pool_plan(c.C, c.H, c.W, c.R, (P, P), argmax16=not wide)
    assert (plan["fwd"], plan["bwd"]) == (fwd_form, bwd_form), (name, P, wide, plan)
    out_r, arg_r = rp.case_ref(name, P)
    if fwd_runs:
        out, arg, arg_dev = forward(c, P, wide)
        assert np.array_equal(arg, arg_r), (name, P, wide, "argmax", int((arg != arg_r).sum()))
        assert_same(name, "out (%d x %d bins, %s argmax)" % (P, P, "int32" if wide else "16-bit"), out, out_r)
    else:                                                                    # the forward cannot produce it: the reference's argmax
        arg_dev = T(arg_r) if wide else arg16_dev(arg_r)
    if bwd_form is not None:
        got = backward(c, P, wide, c.go(P, P), arg_dev)
        assert_same(name, "grad_feat (%s, %s argmax)" % (bwd_form, "int32" if wide else "16-bit"), got, rp.case_bwd(name, P)[0].astype(F))
    return plan


def bwd16_form(c):
    return "shared_cb" if c.C % 2 else "private8"


# ---------------------------------------------------------------------------------------------- A, B: geometry and values
@pytest.mark.parametrize("name", rp.GEO_CASES + rp.VALUE_CASES)
def test_geometry_and_values_on_both_forwards_and_both_argmax_widths(ops, name):
    """Coordinates on halves (directly, through 0.0625 and through the non-dyadic 0.3), every side pair 1 .. 14, the fp32 artefact sides 57
    and 114, inverted / outside / oversized / one-cell boxes; NaN, +-inf, plateaus and signed zeros: the LDS forward in both argmax widths,
    the generic forward through a 5 x 5 grid, and the backward from each argmax (-1 bins add nothing)."""
    c = rp.case(name)
    check_pair(ops, name, 7, False, "lds", bwd16_form(c))
    check_pair(ops, name, 7, True, "lds", "shared_cb")
    check_pair(ops, name, 5, True, "generic", "shared_cb")


# ---------------------------------------------------------------------------------------------- C: forward launch geometry
@pytest.mark.parametrize("C_,R", rp.LAUNCH_CR)
def test_forward_launch_geometry(ops, C_, R):
    """(S, RB, exclusive) as tests/roi_pool_ref.py LAUNCH_GEOMETRY lists them: workgroups of unequal RoI counts, the task queue's first refill
    (1029 tasks), RB = 256, the non-exclusive LDS request, the channel tails."""
    name = "launch:C%d/R%d" % (C_, R)
    c = rp.case(name)
    for wide in (False, True):
        p = check_pair(ops, name, 7, wide, "lds", "shared_cb" if wide else bwd16_form(c))
        assert (p["S"], p["RB"], p["exclusive"]) == rp.LAUNCH_GEOMETRY[(C_, R)], p


# ---------------------------------------------------------------------------------------------- D: plane-size seams
@pytest.mark.parametrize("H,W", rp.STAGING_SHAPES)
def test_staging_loop_seams(ops, H, W):
    name = "plane:%dx%d" % (H, W)
    hw = H * W
    check_pair(ops, name, 7, False, "lds", "private8" if hw <= 2528 else "private4")
    check_pair(ops, name, 7, True, "lds", "shared_cb")


def refused(fn, *args):
    """The entry point returns an error code (and says why) without launching: the caller checks that its outputs kept their fill."""
    rc = fn(*args)
    assert rc == -1 and L().lib.frcnn_last_error(), rc


def test_one_pixel_past_the_lds_forward(ops):
    """H * W = 3073: the 16-bit forward refuses and launches nothing, the int32 entry takes the generic kernel, and ops.roi_pool gives the
    reference's bits on both sides of the limit (3072: the 16-bit pair; 3073: the int32 pair)."""
    H, W = rp.LIMIT_SHAPE
    name = "plane:%dx%d" % (H, W)
    c = rp.case(name)
    lib = L().lib
    for fill in (0xFF, 0x00):
        with guarded.guarded(fill) as g:
            feat, rois = g.place(T(c.feat)), g.place(T(c.rois))
            out = torch.empty((c.R, c.C, 7, 7), dtype=torch.float32, device=DEV)
            arg = torch.empty((c.R, c.C, 7, 7), dtype=torch.uint16, device=DEV)
            refused(lib.frcnn_roi_pool_fwd_a16, feat.data_ptr(), c.C, H, W, rois.data_ptr(), c.R, 1.0, out.data_ptr(), arg.data_ptr(), stream())
            torch.cuda.synchronize()
            assert bool((out.view(torch.uint8) == fill).all()) and bool((arg.view(torch.uint8) == fill).all())
    check_pair(ops, name, 7, True, "generic", "shared_cb")
    check_pair(ops, name, 7, False, None, "private4", fwd_runs=False)
    for n in ("plane:48x64", name):
        autograd_case(ops, n)


@pytest.mark.parametrize("H,W", list(rp.BWD16_SHAPES))
def test_backward_plane_size_seams_16_bit(ops, H, W):
    name = "plane:%dx%d" % (H, W)
    c = rp.case(name)
    form = rp.BWD16_SHAPES[(H, W)]
    fits = 16 * H * W <= 48 * 1024
    p = check_pair(ops, name, 7, False, "lds" if fits else None, form, fwd_runs=fits)
    assert p["bwd_lds"] == rp.BWD_LDS.get(("a16", (H, W)), p["bwd_lds"])
    if form is None:                                                         # 8193 pixels: refused, nothing launched
        go, arg = T(c.go()), arg16_dev(rp.case_ref(name)[1])
        for fill in (0xFF, 0x00):
            with guarded.guarded(fill) as g:
                g_o, a, rois = g.place(go), g.place(arg), g.place(T(c.rois))
                gf = torch.empty((c.C, H, W), dtype=torch.float32, device=DEV)
                refused(L().lib.frcnn_roi_pool_bwd_a16, g_o.data_ptr(), a.data_ptr(), rois.data_ptr(), 1.0, c.R, c.C, H, W, gf.data_ptr(), stream())
                torch.cuda.synchronize()
                assert bool((gf.view(torch.uint8) == fill).all())


@pytest.mark.parametrize("H,W", list(rp.BWD32_SHAPES))
def test_backward_plane_size_seams_int32(ops, H, W):
    """shared_cb at exactly 65 536 B, the one-channel kernel through its plane-size condition (and at exactly 65 536 B), and the global-atomic
    form, whose memset is what makes grad_feat "fully overwritten": the 0xFF and the 0x00 run must agree on every pixel."""
    name = "plane:%dx%d" % (H, W)
    p = check_pair(ops, name, 7, True, "generic", rp.BWD32_SHAPES[(H, W)])
    assert p["bwd_lds"] == rp.BWD_LDS.get(("i32", (H, W)), p["bwd_lds"])


def test_16_bit_backward_without_boxes_gives_the_same_bits(ops):
    """rois = NULL: every RoI adds with LDS atomics inside the wave-private planes; integer dOut, so the same bits."""
    for name in ("rank:C2/24x24/R64", "rank:C6/24x106/R65"):
        c = rp.case(name)
        assert ops.roi_pool_plan(c.C, c.H, c.W, c.R, have_rois=False)["bwd"] in ("private8", "private4")
        assert not ops.roi_pool_plan(c.C, c.H, c.W, c.R, have_rois=False)["rank_adds"]
        got = backward(c, 7, False, c.go(), arg16_dev(rp.case_ref(name)[1]), with_rois=False)
        assert_same(name, "grad_feat without boxes", got, rp.case_bwd(name)[0].astype(F))


def test_shared_plane_switch_in_a_child_process_gives_the_same_bits(ops):
    """FRCNN_ROI_BWD_SHARED=1 on an even-C 16-bit case: the shared-plane kernel with 16-bit argmax at even C (the plan in the child says so)."""
    name = "rank:C6/24x24/R129"
    code = ("import sys, numpy as np, torch; import roi_pool_ref as rp; from faster_rcnn_pytorch_amd import ops;"
            "c = rp.case(sys.argv[2]); assert ops.roi_pool_plan(c.C, c.H, c.W, c.R)['bwd'] == 'shared_cb';"
            "ft = torch.from_numpy(c.feat[None]).cuda().requires_grad_(True);"
            "out = ops.roi_pool(ft, torch.from_numpy(c.rois).cuda(), (7, 7), c.scale); out.backward(torch.from_numpy(c.go()).cuda());"
            "np.save(sys.argv[1] + '/out.npy', out.detach().cpu().numpy()); np.save(sys.argv[1] + '/g.npy', ft.grad[0].cpu().numpy())")
    assert ops.roi_pool_plan(6, 24, 24, 129)["bwd"] == "private8"
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, FRCNN_ROI_BWD_SHARED="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
        subprocess.run([sys.executable, "-c", code, d, name], check=True, env=env, timeout=300)
        assert_same(name, "out in the child", np.load(os.path.join(d, "out.npy")), rp.case_ref(name)[0])
        assert_same(name, "grad_feat in the child", np.load(os.path.join(d, "g.npy")), rp.case_bwd(name)[0].astype(F))


# ---------------------------------------------------------------------------------------------- E: the rank scheme
@pytest.mark.parametrize("C_,hw,R", rp.RANK_CASES)
def test_rank_scheme_on_distinct_values_with_shared_maxima_everywhere(ops, C_, hw, R):
    """All nine shapes of shared maximum at every bin position (test_roi_pool_ref_host.py), rank and atomic RoIs interleaved in a wave's batch,
    R around the wave-batch of NW * 16 (waves without a RoI must still zero their planes).  Integer dOut: float32(ref64) in every bit.
    dOut ~ randn: two runs bit-identical (the header's promise for even C), and per pixel |got - ref64| <= gamma(n - 1) * sum |g_i|, n = the
    terms the reference scattered there: the bound of ANY order of n fp32 additions (roi_pool_ref.gamma), derived, not measured."""
    name = "rank:C%d/%dx%d/R%d" % (C_, hw[0], hw[1], R)
    c = rp.case(name)
    form = "private8" if hw == rp.RANK_NW8_HW else "private4"
    p = check_pair(ops, name, 7, False, "lds", form)
    assert p["rank_adds"]
    arg = arg16_dev(rp.case_ref(name)[1])
    go = c.go_float()
    a, b = backward(c, 7, False, go, arg), backward(c, 7, False, go, arg)
    assert np.array_equal(bits(a), bits(b))
    ref, n, mag = rp.bwd64(go, rp.case_ref(name)[1], c.C, c.H, c.W)
    err = np.abs(a.astype(np.float64) - ref)
    bound = rp.gamma(np.maximum(n - 1, 0)) * mag
    print("PARITY roi_pool_bwd %s: worst err / bound %.3f, most terms on a pixel %d" % (name, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))), n.max()))
    assert not bits(a)[n == 0].any()                                         # +0.0 where no term exists
    assert (err <= bound).all(), (name, float(err.max()))


# ---------------------------------------------------------------------------------------------- through autograd
def autograd_case(ops, name):
    c = rp.case(name)
    ft = T(c.feat[None]).requires_grad_(True)
    out = ops.roi_pool(ft, T(c.rois), (7, 7), c.scale)
    assert_same(name, "ops.roi_pool", out.detach().cpu().numpy(), rp.case_ref(name)[0])
    out.backward(T(c.go()))
    assert_same(name, "ops.roi_pool backward", ft.grad[0].cpu().numpy(), rp.case_bwd(name)[0].astype(F))


@pytest.mark.parametrize("name", ["geo:kinds/C2", "geo:scale0.3/C3", "values:/C2", "launch:C512/R42", "plane:48x106", "rank:C2/24x24/R64"])
def test_one_case_per_family_through_autograd(ops, name):
    autograd_case(ops, name)
