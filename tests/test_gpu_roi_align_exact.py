"""RoIAlign and RoIPool backward (and the RoIAlign forward) against float64, bit for bit on exact data and inside a derived bound on
general data.  The reference, the exact regime and the cases live in tests/roi_align_ref.py and are proved on the CPU by
tests/test_roi_align_ref_host.py (reference = C oracle in every bit on the exact cases; every list length, segment count, plan and empty
tile a case claims).  On exact data every product and partial sum is an fp32 number, so no summation order, tiling, segmenting or atomic
can change a bit: the expectation everywhere is float32(ref64), compared on the BIT PATTERNS (-0.0 is not 0.0; a NaN left from the
prefill equals nothing).  Gradient buffers are prefilled with NaN and the workspace with 0xFF bytes.
Run on the GPU box:  python -m pytest tests/test_gpu_roi_align_exact.py -m gpu -s
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import roi_align_ref as ra
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want64):
    return np.array_equal(bits(got), bits(np.asarray(want64).astype(np.float32)))


class Bwd:
    """frcnn_ms_roi_align_bwd through the C ABI on buffers of its own: NaN in the gradient planes, 0xFF in the workspace."""

    def __init__(self, shapes, scales, Cc, R_max):
        from faster_rcnn_pytorch_amd import _lib
        self.lib, self.check = _lib.lib, _lib.check
        self.shapes, self.C = shapes, Cc
        self.H = np.array([s[0] for s in shapes], np.int32)
        self.W = np.array([s[1] for s in shapes], np.int32)
        self.sc = np.array(scales, np.float32)
        self.grads = [torch.empty((Cc, h, w), dtype=torch.float32, device=DEV) for h, w in shapes]
        self.ptrs = (C.c_void_p * len(shapes))(*[g.data_ptr() for g in self.grads])
        nb = self.lib.frcnn_ms_roi_align_bwd_workspace(self.H.ctypes.data, self.W.ctypes.data, len(shapes), Cc, R_max)
        self.ws = torch.full((max(nb, 256),), 0xFF, dtype=torch.uint8, device=DEV)

    def call(self, go_dev, rois_dev, R, PH=7, SR=2, aligned=False):
        """Enqueues prefill + backward on the current stream; no sync.  go_dev / rois_dev stay alive with the caller."""
        for g in self.grads:
            g.fill_(float("nan"))
        need = self.lib.frcnn_ms_roi_align_bwd_workspace(self.H.ctypes.data, self.W.ctypes.data, len(self.shapes), self.C, R)
        assert need <= self.ws.numel()
        self.check(self.lib.frcnn_ms_roi_align_bwd(go_dev.data_ptr(), self.ptrs, self.H.ctypes.data, self.W.ctypes.data, self.sc.ctypes.data,
                                                   len(self.shapes), self.C, rois_dev.data_ptr(), R, PH, PH, SR, int(aligned), 2, 224.0, 4,
                                                   self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream().cuda_stream), "ms_roi_align_bwd")

    def result(self):
        torch.cuda.synchronize()
        return [g.cpu().numpy() for g in self.grads]


def run_case(c, misalign=False):
    b = Bwd(c.shapes, c.scales, c.C, c.R)
    rois = T(c.rois)
    if misalign:                  # grad_out one float into a larger buffer: 4 mod 16
        buf = torch.zeros((c.go.size + 8,), dtype=torch.float32, device=DEV)
        go = buf[1:1 + c.go.size]
        go.copy_(T(c.go).reshape(-1))
        assert go.data_ptr() % 16 == 4
    else:
        go = T(c.go)
        assert go.data_ptr() % 16 == 0
    b.call(go, rois, c.R, c.PH, c.SR, c.aligned)
    return b.result()


# Which branch a case reaches (asserted on the CPU by test_roi_align_ref_host.py from the lists the reference's footprints give):
#   seg:N        ONE 16 x 8 tile owns all N RoIs.  1, 32: one item, tile written straight to the plane.  33, 64: 2 segments, 65: 3 -- partial
#                tiles through the workspace, the last arriver adds them in segment order.  1024: 32 segments of 32; 1025: 32 of 32 / 33 (the
#                segment count is capped).  2080: 32 of 65 -- second trip of the 64-entry chunk loop with ONE entry; 2081: one segment of 66.
#   chunk:R      lists kernel: R = 255, 256, 257, 513 around its 256-RoI chunks; the last chunk's RoIs append to lists the first began.
#   regC:C       C = 3, 33, 40: register instantiation, partial last channel group.   dma64: C = 64, LDS-DMA instantiation.
#   mixed:       RoIs with records (<= 16 tiles) and with tables built in the tile kernel (> 16) alternate in the same lists, DMA path.
#   coarsen:     512 RoIs over most of a 50 x 84 level: more segments than the item table holds, the plan doubles the split threshold.
#   pyr:64       four levels, R = 600: item blocks < 1280 = one round of resident workgroups, fill blocks last in the grid.
#   pyr:128      the same at C = 128: item blocks > 1536, fill blocks INSIDE the grid.  Both have tiles no RoI touches (zero-filled).
#   pyr_empty:   level 0 without a RoI.      shape:HxW  levels smaller than, equal to and one past a tile; 13 x 21 and 25 x 42.
#   aligned:*    aligned = 1 (positions b * scale - 0.5, no clamp of the size) on the DMA path (four levels) and the register path.
#   generic:P/S  (P x P bins, sampling ratio S) != (7, 2): roi_align_bwd_kernel, memset + fp32 atomics -- exact data makes them order-free.
TILE_CASES = [n for n in ra.EXACT_CASES if not n.startswith(("generic", "b2b"))]


@pytest.mark.parametrize("name", TILE_CASES + [n for n in ra.EXACT_CASES if n.startswith("generic")])
def test_backward_equals_float64_in_every_bit(ops, name):
    c = ra.case(name)
    ra.check_premise(name)                                                        # sum of magnitudes < 2^24 units: every order is exact
    if len(c.shapes) > 1:
        assert np.array_equal(ops.roi_level_map(T(c.rois)).cpu().numpy(), c.level)
    got = run_case(c)
    for l, (g, _) in enumerate(ra.case_ref(name)):
        bad = bits(got[l]) != bits(g.astype(np.float32))
        assert not bad.any(), "%s level %d: %d of %d values differ, first at %s" % (name, l, bad.sum(), bad.size, np.argwhere(bad)[0])


def test_misaligned_grad_out_takes_the_register_path_with_whole_groups_and_gives_the_same_bits(ops):
    c = ra.case("dma64:")
    a, m = run_case(c), run_case(c, misalign=True)
    ref = ra.case_ref("dma64:")[0][0]
    assert same_bits(a[0], ref) and same_bits(m[0], ref) and np.array_equal(bits(a[0]), bits(m[0]))


@pytest.mark.parametrize("name", ["pyr:64", "aligned:one", "generic:8/0"])
def test_backward_through_autograd_equals_float64_in_every_bit(ops, name):
    c = ra.case(name)
    fts = [torch.zeros((1, c.C, h, w), device=DEV, requires_grad=True) for h, w in c.shapes]
    ops.ms_roi_align(fts, T(c.rois), c.PH, c.SR, scales=c.scales, aligned=c.aligned).backward(T(c.go))
    for l, (g, _) in enumerate(ra.case_ref(name)):
        assert same_bits(fts[l].grad[0].cpu().numpy(), g), (name, l)


def test_records_switched_off_in_a_child_process_gives_the_same_bits(ops):
    """FRCNN_RA_RECORDS is read once per process: a fresh child builds every weight table inside the tile kernel."""
    code = ("import sys, numpy as np, torch; import roi_align_ref as ra; from faster_rcnn_pytorch_amd import ops;"
            "c = ra.case('mixed:'); ft = torch.zeros((1, c.C, 50, 84), device='cuda', requires_grad=True);"
            "ops.ms_roi_align([ft], torch.from_numpy(c.rois).cuda(), 7, 2, scales=c.scales).backward(torch.from_numpy(c.go).cuda());"
            "np.save(sys.argv[1], ft.grad[0].cpu().numpy())")
    ref = ra.case_ref("mixed:")[0][0]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "g.npy")
        env = dict(os.environ, FRCNN_RA_RECORDS="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
        subprocess.run([sys.executable, "-c", code, out], check=True, env=env, timeout=300)
        assert same_bits(np.load(out), ref)


def test_back_to_back_calls_on_one_workspace_without_a_sync(ops):
    """R = 600 -> 5 -> 0 -> 600 on ONE workspace and the same gradient planes, nothing but stream order in between: the tickets (the plan's in
    the library, the tiles' in the workspace) must be left ready by each call.  The planes are copied on the stream after each call."""
    c = ra.case("b2b:")
    b = Bwd(c.shapes, c.scales, c.C, c.R)
    go, rois = T(c.go), T(c.rois)
    snaps = []
    for R in (600, 5, 0, 600):
        b.call(go, rois, R)
        snaps.append((R, [g.clone() for g in b.grads]))
    torch.cuda.synchronize()
    for k, (R, gs) in enumerate(snaps):
        ra.check_premise("b2b:", R)
        for l, (g, _) in enumerate(ra.case_ref("b2b:", R)):
            got = gs[l].cpu().numpy()
            assert same_bits(got, g), "call %d (R = %d) level %d" % (k, R, l)
            if R == 0:
                assert not bits(got).any()                                          # all +0.0


FWD_C = 40          # one whole 32-channel group and a partial one


@pytest.mark.parametrize("name", ["pyr:64", "aligned:pyr", "aligned:one", "shape:1x3", "shape:17x9", "mixed:", "generic:4/2", "generic:7/4", "generic:8/0"])
def test_forward_equals_float64_in_every_bit(ops, name):
    """Integer features on the dyadic RoIs: roi_align_fwd77_kernel (footprints staged in LDS in one or several channel passes) and the generic
    forward equal fwd64 in every bit -- arithmetic, not a restatement of the oracle's loop."""
    c = ra.case(name)
    rng = np.random.RandomState(len(name))
    feats = [rng.randint(-8, 9, (FWD_C, h, w)).astype(np.float32) for h, w in c.shapes]
    want = sum(ra.fwd64(f, c.rois, s, c.aligned, c.level, l, c.PH, c.SR) for l, (f, s) in enumerate(zip(feats, c.scales)))
    assert np.abs(want).max() / c.unit < 2 ** 24 and np.array_equal(np.round(want / c.unit), want / c.unit)
    out = ops.ms_roi_align([T(f[None]) for f in feats], T(c.rois), c.PH, c.SR, scales=c.scales, aligned=c.aligned)
    assert same_bits(out.cpu().numpy(), want + 0.0)


# ---------------------------------------------------------------------------------------------- RoIPool backward
@pytest.mark.parametrize("Cc", [64, 512])
def test_roi_pool_backward_integer_gradients_equal_the_float64_scatter_in_every_bit(ops, Cc):
    """The piecewise-constant map of test_roi_pool_backward_duplicate_maxima_... (bins sharing their maximum all over), integer dOut: every
    order of the wave-private planes' read-modify-write adds (and of the int32 ABI's LDS atomics) is exact."""
    from faster_rcnn_pytorch_amd import _lib
    rng = np.random.RandomState(5 + Cc)
    H, W, R = 37, 62, 128
    f = np.repeat(np.repeat(rng.randn(Cc, 10, 16).astype(np.float32), 4, axis=1), 4, axis=2)[:, :H, :W].copy()
    f[::3] += (rng.randn(Cc // 3 + 1, H, W) * 0.01).astype(np.float32)[:len(f[::3])]
    wh = rng.rand(R, 2) * np.array([0.9, 0.9]) + 0.02
    ctr = rng.rand(R, 2)
    rois = (np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).clip(0, 1) * np.array([W, H, W, H])).astype(np.float32)
    rois[0] = [3, 2, 9, 8]
    rois[1] = [3, 2, 10, 9]
    rois[2] = [5, 5, 6, 6]
    rois[3] = [20, 10, 26, 30]
    rois[4] = [W + 2, H + 2, W + 5, H + 5]
    rois[5] = [0, 0, W, H]
    out_o, arg_o = orc.roi_pool_fwd(f, rois, 7, 7, 1.0)
    go = rng.randint(-8, 9, out_o.shape).astype(np.float32)
    a = arg_o.reshape(R, Cc, 49).astype(np.int64)
    flat = (np.arange(Cc)[None, :, None] * (H * W) + a)[a >= 0]
    want = np.bincount(flat, weights=go.reshape(R, Cc, 49).astype(np.float64)[a >= 0], minlength=Cc * H * W).reshape(Cc, H, W) + 0.0
    assert (arg_o[4] == -1).all() and np.abs(want).max() < 2 ** 24
    ft = T(f[None]).requires_grad_(True)
    out = ops.roi_pool(ft, T(rois), (7, 7), 1.0)
    assert np.array_equal(out.detach().cpu().numpy(), out_o)
    out.backward(T(go))
    assert same_bits(ft.grad[0].cpu().numpy(), want)
    out32, arg32 = ops.roi_pool_with_argmax(T(f[None]), T(rois), (7, 7), 1.0)
    assert np.array_equal(arg32.cpu().numpy(), arg_o)
    gf = torch.full((1, Cc, H, W), float("nan"), dtype=torch.float32, device=DEV)
    got = T(go)
    _lib.check(_lib.lib.frcnn_roi_pool_bwd(got.data_ptr(), arg32.data_ptr(), R, Cc, H, W, 7, 7, gf.data_ptr(), torch.cuda.current_stream().cuda_stream), "roi_pool_bwd")
    torch.cuda.synchronize()
    assert same_bits(gf[0].cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- general data: a derived per-pixel bound
@pytest.mark.parametrize("name", ["pyr", "one"])
def test_backward_general_data_within_the_derived_bound_of_float64(ops, name):
    """Non-dyadic, log-uniform RoIs (with the partly-outside, whole-frame, 1 x 1-clamped and corner-clamp boxes), dOut ~ randn:
    |got - ref64| <= (n_l + 48) * 2^-24 * absgrad at EVERY pixel (derivation: roi_align_ref.bound_units), exactly zero where absgrad is.
    'pyr': C = 64 on the four-level 672 x 400 pyramid, R = 512 (LDS-DMA path); 'one': one 50 x 84 level, C = 40 (register path).
    Measured on an MI355X: see docs/PARITY.md."""
    c = ra.general_case(name)
    got = run_case(c)
    for l, (g, a) in enumerate(ra.general_ref(name)):
        n_l = int((c.level == l).sum())
        o = got[l].astype(np.float64)
        err = np.abs(o - g)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(a > 0, err / (2.0 ** -24 * a), 0.0)
        print("PARITY roi_align_bwd general %s level %d: n_l %d, worst err %.2f x 2^-24 absgrad (bound %d)" % (name, l, n_l, np.nanmax(q), ra.bound_units(n_l)))
        assert not bits(got[l])[a == 0].any(), "non-zero (or -0.0, or NaN) where no term exists"
        assert (err <= ra.bound_units(n_l) * 2.0 ** -24 * a).all(), (name, l, float(np.nanmax(q)))
