"""CPU-only checks of the fused detection post-process boundary (frcnn_detect_postprocess): workspace sizing, the symbol's
declaration / export / binding, and the op layer's refusal of CPU tensors."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def test_detect_workspace_is_positive_and_monotone_inside_the_limits_and_zero_outside(L):
    assert L.OP_DETECT == 11
    prev = 0
    for P in (1, 7, 300, 1000, 2000, 2048):
        row = [L.workspace_bytes(L.OP_DETECT, P, C) for C in (2, 3, 21, 91, 256)]
        assert all(b > 0 for b in row) and row == sorted(row)
        assert row[0] >= prev
        prev = row[0]
        assert row[-1] >= 255 * P * (16 + 4 + 4)                 # boxes, scores and kept rows of every class
    for P, C in ((0, 21), (2049, 21), (300, 1), (300, 257), (-1, 21)):
        assert L.workspace_bytes(L.OP_DETECT, P, C) == 0
    assert L.workspace_bytes(99, 1, 1) == 0


def test_detect_symbol_is_declared_exported_and_bound(L):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frcnn_hip.h")).read(), flags=re.S)
    assert re.search(r"\bfrcnn_detect_postprocess\s*\(", txt)
    assert re.search(r"FRCNN_OP_DETECT\s*=\s*11\b", txt)
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    assert " T frcnn_detect_postprocess" in out
    assert "frcnn_detect_postprocess" in L.SIGNATURES and len(L.SIGNATURES["frcnn_detect_postprocess"][1]) == 18
    assert L.lib.frcnn_abi_version() == 7


def test_detect_refusals_without_a_device(L):
    """Limits and NULL pointers are checked before anything is launched."""
    f = L.lib.frcnn_detect_postprocess
    args = lambda P, C: [None] * 4 + [P, C, 0.05, None, 0.3] + [None] * 7 + [0, None]   # noqa: E731
    assert f(*args(2049, 21)) == -2 and f(*args(300, 257)) == -2 and f(*args(0, 21)) == -2 and f(*args(300, 1)) == -2
    assert f(*args(300, 21)) == -1 and b"NULL" in L.lib.frcnn_last_error()


def test_detect_postprocess_refuses_cpu_tensors(L):
    import torch
    from faster_rcnn_pytorch_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.detect_postprocess(torch.zeros(4, 3), torch.zeros(4, 12), torch.zeros(4, 4), torch.full((1,), 4, dtype=torch.int32), 0.05)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.detect_postprocess(torch.zeros(4, 3, dtype=torch.bfloat16), torch.zeros(4, 12), torch.zeros(4, 4),
                               torch.full((1,), 4, dtype=torch.int32), 0.05)
