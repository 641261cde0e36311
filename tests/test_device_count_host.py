"""CPU-only checks of the device-count path: the two new entry points are declared, exported and bound with the documented argument
lists, the operators and both mirrors take the new keywords, and parallel.FrameSlot refuses what the host can see."""
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frcnn_hip.h")


@pytest.fixture(scope="module")
def L():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def _declaration(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m, "%s is not declared in include/frcnn_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_entry_points_are_declared_exported_and_bound(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    for name in ("frcnn_rpn_targets_n", "frcnn_head_targets_n"):
        assert re.search(r" T %s\b" % name, out), name
        assert name in L.SIGNATURES and hasattr(L.lib, name)
        assert len(L.SIGNATURES[name][1]) == len(_declaration(name)), name
    # the classic entry points stay, with the argument lists they had; the new ones add exactly the count (and the head maker's `empty`)
    assert len(_declaration("frcnn_rpn_targets_n")) == len(_declaration("frcnn_rpn_targets")) + 1 == 19
    assert len(_declaration("frcnn_head_targets_n")) == len(_declaration("frcnn_head_targets")) + 2 == 26
    assert _declaration("frcnn_rpn_targets_n")[5] == "const int32_t *n_gt_dev"
    assert _declaration("frcnn_head_targets_n")[7] == "const int32_t *n_gt_dev"
    assert _declaration("frcnn_head_targets_n")[-2:] == ["int32_t *empty_dev", "void *stream"]
    assert L.lib.frcnn_abi_version() == L.ABI_VERSION == 7                     # entry points were only added
    txt = open(HEADER).read()
    assert re.search(r"#define\s+FRCNN_HT_ERR_GT_COUNT\s+16\b", txt) and re.search(r"#define\s+FRCNN_RPN_ERR_GT_COUNT\s+16\b", txt)
    assert L.HT_ERR_GT_COUNT == L.RPN_ERR_GT_COUNT == 16


def test_the_new_entry_points_validate_without_a_device(L):
    rc = L.lib.frcnn_rpn_targets_n(0, None, 10, None, 0, None, None, 0, None, 0, 0, 0, None, None, None, None, None, 0, None)
    assert rc == -1 and b"G must be >= 1" in L.lib.frcnn_last_error()
    rc = L.lib.frcnn_rpn_targets_n(0, None, 10, None, 4097, None, None, 0, None, 0, 0, 0, None, None, None, None, None, 0, None)
    assert rc == -1 and b"above limit 4096" in L.lib.frcnn_last_error()
    rc = L.lib.frcnn_head_targets_n(0, None, None, 300, None, None, 0, None, 1, 32, 128, None, 0, None, 0, 0, 0, None, None, None, None, None, None, None,
                                    None, None)
    assert rc == -1 and b"G >= 1" in L.lib.frcnn_last_error()
    rc = L.lib.frcnn_head_targets_n(0, None, None, 4000, None, None, 97, None, 1, 32, 128, None, 0, None, 0, 0, 0, None, None, None, None, None, None, None,
                                    None, None)
    assert rc == -2 and b"above limit 4096" in L.lib.frcnn_last_error()


def test_operators_and_mirrors_take_the_keywords(L):
    from faster_rcnn_pytorch_amd import model, new_model, ops
    assert inspect.signature(ops.rpn_targets).parameters["n_gt"].default is None
    p = inspect.signature(ops.head_targets).parameters
    assert p["n_gt"].default is None and p["empty"].default is None
    for m in (model, new_model):
        p = inspect.signature(m.FRCNN.forward).parameters
        assert list(p)[4:] == ["n_gt", "empty"] and p["n_gt"].default is None and p["empty"].default is None
        assert inspect.signature(m.RPNTargetMaker.forward).parameters["n_gt"].default is None
    for cls in (model.FastRcnnTargetMaker, new_model.FRCNNTargetMaker):
        p = inspect.signature(cls.forward).parameters
        assert p["n_gt"].default is None and p["empty"].default is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rpn_targets(torch.zeros(4, 4), torch.zeros(2, 4), n_gt=torch.zeros(1, dtype=torch.int32))
    assert "ground-truth" in " ".join(ops.describe_status(L.HT_ERR_GT_COUNT))
    assert ops.describe_status(L.HT_ERR_SHORT) == ops.describe_status(L.HT_ERR_SHORT | 32)     # an unknown bit names nothing


def test_frame_slot_argument_checks(L):
    from faster_rcnn_pytorch_amd import parallel
    for bad in (0, -1, 4097, 2.0, True, None):
        with pytest.raises(ValueError, match="gt_capacity"):
            parallel.FrameSlot((32, 48), bad, "cpu")
    for bad in ((0, 48), (32,), 32, (32, -1), None):
        with pytest.raises(ValueError, match="image_hw"):
            parallel.FrameSlot(bad, 4, "cpu")
    slot = parallel.FrameSlot((32, 48), 4, "cpu")                              # plain tensors: the class itself runs anywhere
    assert tuple(slot.x.shape) == (1, 3, 32, 48) and slot.x.dtype == torch.float32
    assert tuple(slot.boxes.shape) == (4, 4) and tuple(slot.labels.shape) == (4,) and slot.labels.dtype == torch.int64
    assert slot.n_gt.dtype == slot.empty.dtype == torch.int32 and slot.n_gt.numel() == slot.empty.numel() == 1
    x, b, l = torch.randn(1, 3, 32, 48), torch.rand(3, 4), torch.tensor([5, 6, 7])
    addresses = [t.data_ptr() for t in (slot.x, slot.boxes, slot.labels, slot.n_gt, slot.empty)]
    with pytest.raises(ValueError, match="one slot serves one input shape"):
        slot.load(torch.randn(1, 3, 32, 50), b, l, 3)
    with pytest.raises(ValueError, match="5 boxes, the slot holds 4"):
        slot.load(x, torch.rand(5, 4), torch.zeros(5, dtype=torch.int64), 5)
    with pytest.raises(ValueError, match=r"boxes must be \[r, 4\]"):
        slot.load(x, torch.rand(3, 5), l, 3)
    with pytest.raises(ValueError, match="need 3 labels"):
        slot.load(x, b, torch.tensor([1, 2]), 2)
    for bad in (4, -1, 2.0, True):
        with pytest.raises(ValueError, match="count"):
            slot.load(x, b, l, bad)
    with pytest.raises(ValueError, match="ONE integer"):
        slot.load(x, b, l, torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="ONE integer"):
        slot.load(x, b, l, torch.tensor([1.0]))
    # what load() does, on plain tensors: copies in place, the tail cleared, the count from an int, a tensor or the row count
    slot.load(x, b, l, 2)
    assert torch.equal(slot.x, x) and torch.equal(slot.boxes[:3], b) and not slot.boxes[3:].any() and slot.labels.tolist() == [5, 6, 7, 0]
    assert slot.n_gt.tolist() == [2]
    slot.load(x[0], b[:1], l[:1], torch.tensor(1, dtype=torch.int64))
    assert slot.n_gt.tolist() == [1] and not slot.boxes[1:].any() and slot.labels.tolist() == [5, 0, 0, 0]
    slot.load(x, b, l)
    assert slot.n_gt.tolist() == [3]
    slot.load(x, b, l, 0)                                                       # a frame without boxes is data, not an error
    assert slot.n_gt.tolist() == [0] and slot.empty.tolist() == [0]             # `empty` belongs to the head target maker
    assert addresses == [t.data_ptr() for t in (slot.x, slot.boxes, slot.labels, slot.n_gt, slot.empty)]
