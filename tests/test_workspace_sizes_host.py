"""Every workspace-size function of libfrcnn_hip.so against a table recorded from a build of the commit BEFORE the host-side layout code
was collected into csrc/frcnn_host.h (tools/dev/record_workspace_sizes.py wrote tests/golden/workspace_sizes.json): frcnn_workspace_bytes
for all sixteen op codes and every exported *_workspace / *_floats / *_words function, at the sizes the models use, the smallest legal
sizes, one size on each side of every internal switch (NMS_CASCADE_MIN, SS_MIN_N, DM_MAX_CAND, C = 2 and DET_MAX_C for detect, ...) and the
refusals that answer 0.  A change to a layout function that moves a size fails here, on a machine without a GPU; the offsets behind the
sizes are the guard-band tests' business (test_gpu_guarded.py).

ctypes only.  The rows that depend on the CU count (OP_RPN_CONV_F32, frcnn_conv3x3_f32_workspace and the two functions sized through the
same carve, frcnn_rpn_conv3x3_f32_workspace and frcnn_gemm_nt_f32_workspace) were recorded with 256 CUs: that is the library's fallback
when there is no device, as on the machine that recorded them, and it is the MI355X's count, so the table holds on both."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")))
ROWS = [(name, args, want) for name, args, want in TABLE["rows"]]


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(so)
    for name, sig in TABLE["sig"].items():
        f = getattr(lib, name)
        f.restype = C.c_size_t
        f.argtypes = [{"i": C.c_int, "q": C.c_int64, "I": C.c_void_p}[c] for c in sig]
    return lib


def call(lib, name, args):
    keep = [(C.c_int32 * len(a))(*a) if isinstance(a, list) else a for a in args]       # `keep` owns the arrays for the call
    return int(getattr(lib, name)(*[C.cast(a, C.c_void_p) if isinstance(a, C.Array) else a for a in keep]))


def test_every_recorded_size_is_unchanged(lib):
    got = [(name, args, call(lib, name, args)) for name, args, _ in ROWS]
    moved = [(name, args, want, have) for (name, args, want), (_, _, have) in zip(ROWS, got) if want != have]
    assert not moved, "%d of %d sizes moved, first: %s%s recorded %d, now %d" % ((len(moved), len(ROWS)) + moved[0])


def test_the_table_covers_what_it_claims():
    """The grid itself: every op code with live rows, both sides of each switch, the refusals, every exported size function."""
    ops = {}
    for name, args, want in ROWS:
        if name == "frcnn_workspace_bytes":
            ops.setdefault(args[0], []).append((args[1], args[2], want))
    assert set(range(1, 17)) <= set(ops)
    for op in range(1, 17):
        assert any(w > 0 for _, _, w in ops[op]), op
        assert (-1, 1, 0) in ops[op] and (1, -1, 0) in ops[op], op                      # a negative argument answers 0
    assert ops[99] == [(1, 1, 0)]
    n1 = lambda op: {a for a, _, _ in ops[op]}                                           # noqa: E731
    assert {4095, 4096, 4097} <= n1(1)                                                   # SS_MIN_N
    assert {16383, 16384, 16385} <= n1(2)                                                # NMS_CASCADE_MIN
    assert {2047, 2048, 2049} <= n1(16)                                                  # DM_MAX_CAND
    assert {2, 256} <= {c for _, c, w in ops[11] if w > 0}                               # detect: C = 2 and DET_MAX_C
    for op in (12, 13, 15):                                                              # a G above the limit answers 0
        assert (100, 1025, 0) in ops[op], op
    assert (300, 257, 0) in ops[11] and (100, 257, 0) in ops[16]
    assert {name for name, _, _ in ROWS} == set(TABLE["sig"])
    assert TABLE["cu_count"] == 256
