"""CPU-only checks of frcnn_conv3x3_f32_bwd (both gradients of a layer in one call): what it refuses is refused through the C ABI before anything is
launched, so none of this touches a device.  The pointers handed over are never dereferenced: every call here ends in its argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3          # include/frcnn_hip.h


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def _i32(v):
    return np.asarray(v, np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class _Call:
    """One call's arguments by name; `fake` stands for a device address that a refused call never follows."""

    def __init__(self, L, H=(40,), W=(52,), Cin=128, Cout=128):
        self.L = L
        self.H, self.W = _i32(H), _i32(W)
        n = len(H)
        fake = C.c_void_p(0x1000)
        levels = (C.c_void_p * n)(*([0x1000] * n))
        self.need = int(L.lib.frcnn_conv3x3_f32_workspace(_p(self.H), _p(self.W), n, Cin, Cout))
        self.kw = dict(dy=levels, bits=None, dx=levels, H=_p(self.H), W=_p(self.W), n=n, Cin=Cin, Cout=Cout, w=fake, urot=None, pooled=0, xt=fake, dyt=fake, dw=fake, db=None,
                       ws=fake, nws=self.need, stream=None)

    def __call__(self, **over):
        k = dict(self.kw, **over)
        return self.L.lib.frcnn_conv3x3_f32_bwd(k["dy"], k["bits"], k["dx"], k["H"], k["W"], k["n"], k["Cin"], k["Cout"], k["w"], k["urot"], k["pooled"], k["xt"], k["dyt"],
                                                k["dw"], k["db"], k["ws"], k["nws"], k["stream"])


def test_null_pointers_are_refused(L):
    call = _Call(L)
    assert call.need > 0
    for name in ("dy", "dx", "H", "W", "w", "ws", "xt", "dyt", "dw"):
        assert call(**{name: None}) == INVALID_ARG, name
        assert b"conv3x3_f32_bwd" in L.lib.frcnn_last_error(), name
    holes = (C.c_void_p * 1)(0)                                      # a level list with a NULL level
    assert call(dy=holes) == INVALID_ARG
    assert call(n=0) == INVALID_ARG and call(n=6) == INVALID_ARG


def test_a_workspace_one_byte_short_is_refused(L):
    for shape in (dict(), dict(H=(37,), W=(62,), Cin=512, Cout=512), dict(H=(24, 12), W=(32, 16), Cin=64, Cout=64)):
        call = _Call(L, **shape)
        assert call(nws=call.need - 1) == WORKSPACE
        assert b"workspace" in L.lib.frcnn_last_error()
        assert call(nws=0) == WORKSPACE


def test_channel_counts_and_pooled_gradients_outside_the_stage_are_refused(L):
    for Cin, Cout in ((96, 128), (128, 96), (32, 64), (0, 64), (8192, 8192)):        # both sides are tiled by 64 in one of the two products
        call = _Call(L, Cin=128, Cout=128)
        assert call(Cin=Cin, Cout=Cout) == UNSUPPORTED, (Cin, Cout)
    small = _Call(L, H=(8,), W=(12,), Cin=512, Cout=512)            # the 2 x 2 tile by the stage's own rule: no fused pooling there
    assert int(L.lib.frcnn_conv3x3_f32_tile_size(_p(small.H), _p(small.W), 1)) == 2
    assert small(pooled=1, bits=C.c_void_p(0x1000)) == UNSUPPORTED
    big = _Call(L)
    assert int(L.lib.frcnn_conv3x3_f32_tile_size(_p(big.H), _p(big.W), 1)) == 4
    assert big(pooled=1, bits=None) == UNSUPPORTED                   # a pooled gradient without the forward's words


def test_workspace_holds_the_second_products_region_and_grows_with_the_layer(L):
    """A launch that holds both products of a backward gives the second one tickets and slabs of its own: frcnn_conv3x3_f32_workspace covers two ticket
    blocks (32768 words each) and, beside the K-major product's two slabs per range (2 ranges per CU), the k-contiguous product's (1 range per CU) --
    with the 256 CUs the library assumes where it finds no device, 96 MB of slabs -- whatever the layer; the rest grows with the map and the channels."""
    fixed = 2 * 32768 * 4 + (2 * 256 + 256) * 2 * 128 * 128 * 4
    sizes = []
    for h, w in ((8, 12), (37, 62), (40, 52), (150, 250)):
        call = _Call(L, H=(h,), W=(w,), Cin=256, Cout=256)
        assert call.need >= fixed
        sizes.append(call.need)
        # the refusal order puts the workspace check in front of the cached transforms: with exactly `need` bytes the remaining refusal is the NULL transform
        assert call(xt=None) == INVALID_ARG and call(nws=call.need - 1) == WORKSPACE
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    by_c = [_Call(L, Cin=c, Cout=c).need for c in (64, 128, 256, 512)]
    assert by_c == sorted(by_c) and by_c[0] < by_c[-1]
