"""CPU-only checks of what the fp32 conv stage's other entry points refuse (frcnn_conv3x3_f32_fwd / _bwd_data / _wgrad and the three frcnn_rpn_conv3x3_f32_*
calls; test_conv_bwd_host.py has the one-call backward): every refusal comes through the C ABI before anything is launched, so none of this touches a
device, and the pointers handed over are never dereferenced.  Each case asserts the error code and that the message names the entry point.  The RPN head's
calls hand over to the stage's (Cin = Cout = C, no bias, no mask) and report under the stage's names, which their own names end in."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3          # include/frcnn_hip.h
MAX_LEVELS = 8                                            # FRCNN_MAX_LEVELS (csrc/frcnn_internal.h)
FAKE = 0x1000                                             # stands for a device address that a refused call never follows

# entry point -> its arguments in ABI order; "a" / "b" are the two per-level pointer lists, "w" the weights (or the weight gradient)
ENTRIES = {
    "conv3x3_f32_fwd": ("a", "b", "H", "W", "n", "Cin", "Cout", "w", "bias", "relu", "bits", "xt", "urot", "ws", "nws", "stream"),
    "conv3x3_f32_bwd_data": ("a", "bits", "b", "H", "W", "n", "Cin", "Cout", "w", "urot", "pooled", "dyt", "want_bias", "ws", "nws", "stream"),
    "conv3x3_f32_wgrad": ("a", "b", "bits", "H", "W", "n", "Cin", "Cout", "w", "dbias", "xt", "pooled", "dyt", "ws", "nws", "stream"),
    "rpn_conv3x3_f32_fwd": ("a", "b", "H", "W", "n", "Cin", "w", "ws", "nws", "stream"),
    "rpn_conv3x3_f32_bwd_data": ("a", "b", "H", "W", "n", "Cin", "w", "ws", "nws", "stream"),
    "rpn_conv3x3_f32_wgrad": ("a", "b", "H", "W", "n", "Cin", "w", "ws", "nws", "stream"),
}
GRADIENTS = [e for e in ENTRIES if not e.endswith("fwd")]


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class _Call:
    """One call of `entry` with its arguments by name; Cin = Cout = C for the RPN head's calls."""

    def __init__(self, L, entry, H=(40,), W=(52,), Cin=128, Cout=128):
        self.L, self.entry = L, entry
        self.fn = getattr(L.lib, "frcnn_" + entry)
        self.name = entry[4:].encode() if entry.startswith("rpn_") else entry.encode()
        self.H, self.W = np.asarray(H, np.int32), np.asarray(W, np.int32)
        n = len(H)
        levels = (C.c_void_p * n)(*([FAKE] * n))
        self.need = int(L.lib.frcnn_conv3x3_f32_workspace(_p(self.H), _p(self.W), n, Cin, Cout))
        self.kw = dict(a=levels, b=levels, H=_p(self.H), W=_p(self.W), n=n, Cin=Cin, Cout=Cout, w=C.c_void_p(FAKE), ws=C.c_void_p(FAKE), nws=self.need, stream=None,
                       bias=None, dbias=None, relu=0, bits=None, xt=None, urot=None, dyt=None, pooled=0, want_bias=0)

    def __call__(self, **over):
        k = dict(self.kw, **over)
        return self.fn(*[k[name] for name in ENTRIES[self.entry]])

    def refused(self, code, **over):
        rc = self(**over)
        err = self.L.lib.frcnn_last_error()
        assert rc == code, (self.entry, over, rc, err)
        assert self.name in err, (self.entry, over, err)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_pointers_level_counts_and_sizes_are_refused(L, entry):
    call = _Call(L, entry)
    assert call.need > 0
    for name in ("a", "b", "H", "W", "w", "ws"):
        call.refused(INVALID_ARG, **{name: None})
    call.refused(INVALID_ARG, a=(C.c_void_p * 1)(0))                # a level list with a NULL level
    call.refused(INVALID_ARG, n=0)
    call.refused(INVALID_ARG, n=MAX_LEVELS + 1)
    for h in (0, -3):
        bad = np.asarray([h], np.int32)
        call.refused(INVALID_ARG, H=_p(bad))
        call.refused(INVALID_ARG, W=_p(bad))


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_channel_counts_outside_the_stage_are_refused(L, entry):
    call = _Call(L, entry)
    call.refused(UNSUPPORTED, Cin=48)                                # not a multiple of the 32-deep chunk
    call.refused(UNSUPPORTED, Cin=0)
    call.refused(UNSUPPORTED, Cin=4128)
    if entry in GRADIENTS:                                           # the gradients' products tile the input side by 64 ...
        call.refused(UNSUPPORTED, Cin=96)
    if entry in ("conv3x3_f32_fwd", "conv3x3_f32_wgrad"):            # ... the forward's and the weight gradient's the output side (the data gradient only
        call.refused(UNSUPPORTED, Cout=96)                           # chunks that one by 32)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_workspace_one_byte_short_is_refused(L, entry):
    for shape in (dict(), dict(H=(37,), W=(62,), Cin=512, Cout=512), dict(H=(24, 12), W=(32, 16), Cin=256, Cout=256)):
        call = _Call(L, entry, **shape)
        call.refused(WORKSPACE, nws=call.need - 1)
        assert b"workspace" in L.lib.frcnn_last_error()
        call.refused(WORKSPACE, nws=0)


def test_the_forward_refuses_an_activation_it_does_not_know(L):
    call = _Call(L, "conv3x3_f32_fwd")
    call.refused(INVALID_ARG, relu=3)
    call.refused(INVALID_ARG, relu=-1)
    call.refused(WORKSPACE, relu=3, nws=call.need - 1)               # the workspace check comes first


def test_pooled_forms_need_the_4x4_tile_and_the_forwards_words(L):
    bits = C.c_void_p(FAKE)
    small = dict(H=(8,), W=(12,), Cin=512, Cout=512)                 # the 2 x 2 tile by the stage's own rule: no fused pooling there
    probe = _Call(L, "conv3x3_f32_fwd", **small)
    assert int(L.lib.frcnn_conv3x3_f32_tile_size(_p(probe.H), _p(probe.W), 1)) == 2
    probe.refused(UNSUPPORTED, relu=2, bits=bits)
    _Call(L, "conv3x3_f32_bwd_data", **small).refused(UNSUPPORTED, pooled=1, bits=bits)
    _Call(L, "conv3x3_f32_wgrad", **small).refused(UNSUPPORTED, pooled=1, bits=bits)
    big = _Call(L, "conv3x3_f32_bwd_data")
    assert int(L.lib.frcnn_conv3x3_f32_tile_size(_p(big.H), _p(big.W), 1)) == 4
    big.refused(UNSUPPORTED, pooled=1, bits=None)                    # a pooled gradient without the forward's words
