"""tests/guarded.py on the CPU (guard_cpu=True): fake "ops" in plain torch that misbehave in each way the harness exists to catch,
and the assertion that it names the right allocation, side and offset; a well-behaved op passes; and everything it patched is the
original again afterwards, also after an exception."""
import re

import pytest
import torch

import guarded as G
from faster_rcnn_pytorch_amd import _lib, evaluation, ops, transforms

CPU = torch.device("cpu")
N = 37


def _beyond(t, n_before=0, n_after=0):
    """The elements of a flat tensor with n_before in front of it and n_after behind it: what a kernel with a wrong predicate addresses.
    (Inside the arena's storage, so plain torch can do it.)"""
    return torch.as_strided(t, (n_before + t.numel() + n_after,), (1,), t.storage_offset() - n_before)


def good_op(x):
    out = torch.empty_like(x)
    ws = ops._workspace(x.device, 4 * x.numel())
    tmp = ws.view(torch.float32)
    tmp.copy_(x)
    tmp.mul_(2)
    out.copy_(tmp)
    ctrl = ops._ctrl_workspace(x.device, "det_loss", 64)
    ctrl[0] = 1                                         # a ticket taken ...
    ctrl[0] = 0                                         # ... and put back
    ctrl[8] = 5                                         # behind the documented word: the op's own business
    return out


def store_past_end(x):
    out = torch.empty((N,), dtype=torch.float32, device=x.device)
    _beyond(out, n_after=1).copy_(torch.cat([x * 2, x[:1]]))
    return out


def store_before_start(x):
    out = torch.empty((N,), dtype=torch.float32, device=x.device)
    _beyond(out, n_before=1).copy_(torch.cat([x[:1], x * 2]))
    return out


def reads_guard(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    out[N - 1] += _beyond(x, n_after=1)[N].nan_to_num(nan=1.0)          # a padded load without its predicate (NaN -> 1, so that it is a last-bit matter)
    return out


def leaves_one_unwritten(x):
    out = torch.empty_like(x)
    out[:N - 1] = x[:N - 1] * 2
    return out


def scratch_one_byte_over(x):
    out = torch.empty_like(x)
    ws = ops._workspace(x.device, 100)
    _beyond(ws, n_after=1)[100] = 7
    out.copy_(x * 2)
    return out


def bypasses(x):
    return torch.ones(N) * 2 * x                        # not one of the patched constructors: the result is torch's own allocation


def _x():
    return torch.arange(1, N + 1, dtype=torch.float32)


def _case(op):
    def case(g):
        return {"out": op(g.place(_x()))}
    return case


def test_a_well_behaved_op_passes_and_its_tensors_are_arena_views():
    with G.guarded(0xFF, guard_cpu=True) as g:
        x = g.place(_x())
        out = good_op(x)
        g.outputs(out=out)
        z = torch.zeros((3, 5), dtype=torch.int32)
        f = torch.full((4,), 2.5)
        e = torch.empty(2, 3, dtype=torch.int16)
        zl = torch.zeros_like(x, dtype=torch.float64)
        assert all(g.arena_of(t) is not None for t in (x, out, z, f, e, zl))
        assert all(t.is_contiguous() and t.data_ptr() % 64 == 0 for t in (x, out, z, f, e, zl))
        assert int(z.abs().sum()) == 0 and f.tolist() == [2.5] * 4 and zl.dtype == torch.float64 and float(zl.abs().sum()) == 0
        assert e.reshape(-1).tolist() == [-1] * 6       # empty: every integer is -1 under 0xFF ...
        assert bool(torch.isnan(torch.empty(3)).all())  # ... and every float a NaN
        assert g.arena_of(torch.ones(3)) is None
    assert torch.equal(out, _x() * 2)
    ff, zz = G.run_both(_case(good_op), guard_cpu=True)
    assert torch.equal(ff["out"], _x() * 2) and torch.equal(zz["out"], _x() * 2)


def test_a_store_one_element_past_the_end_is_named():
    with pytest.raises(G.GuardError) as e:
        with G.guarded(0xFF, guard_cpu=True) as g:
            g.outputs(out=store_past_end(g.place(_x())))
    msg = str(e.value)
    assert len(msg.splitlines()) == 1
    assert re.search(r"guard after the payload touched: 4 bytes, 0 \.\. 3 bytes past the end, of empty \(37,\) float32 \(148 bytes\) "
                     r"allocated at test_guarded_host\.py:\d+ store_past_end", msg), msg


def test_a_store_one_element_before_the_start_is_named():
    with pytest.raises(G.GuardError) as e:
        with G.guarded(0xFF, guard_cpu=True) as g:
            g.outputs(out=store_before_start(g.place(_x())))
    msg = str(e.value)
    assert len(msg.splitlines()) == 1
    assert re.search(r"guard before the payload touched: 4 bytes, 1 \.\. 4 bytes before the start, of empty \(37,\) float32 \(148 bytes\) "
                     r"allocated at test_guarded_host\.py:\d+ store_before_start", msg), msg


def test_a_zero_fill_sees_the_nonzero_bytes_of_a_stray_store():
    """1.0f is 00 00 80 3f: under the 0x00 fill two of its four bytes differ from the guard -- which is why every case runs under both."""
    with pytest.raises(G.GuardError) as e:
        with G.guarded(0x00, guard_cpu=True) as g:
            g.outputs(out=store_past_end(g.place(_x())))
    assert "guard after the payload touched: 2 bytes, 2 .. 3 bytes past the end" in str(e.value)


def test_a_result_that_depends_on_a_guard_byte_is_named():
    with pytest.raises(G.GuardError) as e:
        G.run_both(_case(reads_guard), guard_cpu=True)
    assert re.search(r"output 'out' \(37,\) differs between the 0xFF and the 0x00 run in 1 elements, first at flat element 36 \(75\.0 vs 74\.0\)", str(e.value)), str(e.value)


def test_an_output_element_left_unwritten_is_named():
    with pytest.raises(G.GuardError) as e:
        G.run_both(_case(leaves_one_unwritten), guard_cpu=True)
    assert re.search(r"output 'out' \(37,\) differs between the 0xFF and the 0x00 run in 1 elements, first at flat element 36 \(nan vs 0\.0\)", str(e.value)), str(e.value)
    with G.guarded(0xFF, guard_cpu=True) as g:          # and against a reference the 0xFF run alone shows it: the element is a NaN
        out = leaves_one_unwritten(g.place(_x()))
    assert torch.isnan(out).tolist() == [False] * (N - 1) + [True]


def test_a_scratch_use_one_byte_past_the_requested_size_is_named():
    with pytest.raises(G.GuardError) as e:
        with G.guarded(0xFF, guard_cpu=True) as g:
            g.outputs(out=scratch_one_byte_over(g.place(_x())))
    msg = str(e.value)
    assert len(msg.splitlines()) == 1
    assert re.search(r"guard after the payload touched: 1 bytes, 0 \.\. 0 bytes past the end, of scratch \(100,\) uint8 \(100 bytes\) "
                     r"allocated at test_guarded_host\.py:\d+ scratch_one_byte_over", msg), msg


def test_the_scratch_is_exactly_what_was_asked_for_and_poisoned():
    with G.guarded(0xFF, guard_cpu=True):
        ws = ops._workspace(CPU, 100)
        assert ws.numel() == 100 and ws.dtype == torch.uint8 and ws.tolist() == [255] * 100
        assert transforms._workspace(CPU, 7).numel() == 7
        assert ops._workspace(CPU, 100).data_ptr() != ws.data_ptr()           # a fresh arena per call
        c = ops._ctrl_workspace(CPU, "rpn_targets", 3000)
        assert c.numel() == 3000 and int(c.sum()) == 0
        assert ops._ctrl_workspace(CPU, "rpn_targets", 3000).data_ptr() != c.data_ptr()
    with G.guarded(0x00, guard_cpu=True, keep_ctrl=("rpn_conv_f32",)):
        c = ops._ctrl_workspace(CPU, "rpn_conv_f32", 512)
        assert ops._ctrl_workspace(CPU, "rpn_conv_f32", 512).data_ptr() == c.data_ptr()    # an op that reads what the call before left
        with pytest.raises(G.GuardError, match="kept across calls but was asked for at 512 and then 1024 bytes"):
            ops._ctrl_workspace(CPU, "rpn_conv_f32", 1024)


def test_a_control_word_not_left_zero_is_named():
    with pytest.raises(G.GuardError) as e:
        with G.guarded(0xFF, guard_cpu=True):
            ops._ctrl_workspace(CPU, "det_loss", 32768)[1] = 3
    assert re.search(r"control words not left zero: 1 bytes in 1 \.\. 1 of ctrl\[det_loss\] \(32768,\) uint8 \(32768 bytes\) allocated at "
                     r"test_guarded_host\.py:\d+ test_a_control_word", str(e.value)), str(e.value)


def test_a_returned_tensor_that_bypassed_the_arenas_is_named():
    with pytest.raises(G.GuardError) as e:
        with G.guarded(0xFF, guard_cpu=True) as g:
            g.outputs(out=bypasses(g.place(_x())))
    assert "output 'out' (37,) float32 does not live in an arena" in str(e.value)


def test_several_faults_are_all_reported():
    with pytest.raises(G.GuardError) as e:
        with G.guarded(0xFF, guard_cpu=True) as g:
            x = g.place(_x())
            g.outputs(a=store_past_end(x), b=store_before_start(x), c=bypasses(x))
    assert len(str(e.value).splitlines()) == 3


def _caches():
    return [sorted((repr(k), id(v)) for k, v in d.items()) for d in (ops._WS, ops._CTRL, ops._CTRL_IN_GRAPHS, ops._CONST)]


def _patched():
    return (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, torch.full, ops._workspace, ops._ctrl_workspace, transforms._workspace,
            evaluation._RecordStore._workspace)


def test_everything_patched_is_the_original_again_afterwards():
    before = _patched()
    caches = _caches()
    with G.guarded(0xFF, guard_cpu=True):
        assert all(a is not b for a, b in zip(_patched(), before))
        ops._WS[("x", 0)] = torch.empty(4)              # what a code path that caches its scratch would leave behind
        ops._CTRL[("y", 0)] = torch.zeros(4)
    assert all(a is b for a, b in zip(_patched(), before))
    assert _caches() == caches
    with pytest.raises(ZeroDivisionError):
        with G.guarded(0x00, guard_cpu=True) as g:
            store_past_end(g.place(_x()))               # (the exception is the news, not the guard)
            ops._WS[("x", 0)] = torch.empty(4)
            1 / 0
    assert all(a is b for a, b in zip(_patched(), before))
    assert _caches() == caches
    with pytest.raises(G.GuardError):                   # and after a failed exit check
        with G.guarded(0xFF, guard_cpu=True) as g:
            store_past_end(g.place(_x()))
    assert all(a is b for a, b in zip(_patched(), before))
    assert not torch.isnan(torch.zeros(3)).any() and torch.empty(3).untyped_storage().nbytes() == 12


def test_cpu_allocations_pass_through_untouched_without_the_switch():
    with G.guarded(0xFF) as g:
        t = torch.empty(5)
        z = torch.zeros(5)
        assert g.arena_of(t) is None and g.arena_of(z) is None and t.untyped_storage().nbytes() == 20 and not g.arenas


def _bare(cls):
    """an evaluator with nothing but what _workspace reads (no device needed)"""
    ev = object.__new__(cls)
    ev._ws, ev.device = {}, CPU
    return ev


def test_an_evaluators_workspace_is_exact_and_its_control_words_are_checked():
    D, Gt = 64, 16
    with G.guarded(0xFF, guard_cpu=True) as g:
        voc, coco = _bare(evaluation.DetectionEvaluator), _bare(evaluation.CocoDetectionEvaluator)
        w = voc._workspace(D, Gt)
        assert w.numel() == _lib.workspace_bytes(_lib.OP_EVAL, D, Gt) and int(w.sum()) == 0 and g.arena_of(w).kind == "ctrl"
        assert voc._workspace(D, Gt) is w                               # dedicated: the same block for every update of this evaluator
        assert _bare(evaluation.DetectionEvaluator)._workspace(D, Gt).data_ptr() != w.data_ptr()
        c = coco._workspace(D, Gt)
        assert c.numel() == _lib.workspace_bytes(_lib.OP_COCO_EVAL, D, Gt) and c.tolist() == [255] * c.numel() and g.arena_of(c).kind == "scratch"
        w[256 + evaluation.MAX_THRESHOLDS * Gt * 8] = 9                 # the first byte behind the winner words: the kernel's own scratch
    with pytest.raises(G.GuardError) as e:
        with G.guarded(0xFF, guard_cpu=True):
            _bare(evaluation.DetectionEvaluator)._workspace(D, Gt)[256 + evaluation.MAX_THRESHOLDS * Gt * 8 - 1] = 9          # the last winner byte
    assert re.search(r"control words not left zero: 1 bytes in 2303 \.\. 2303 of ctrl\[eval\]", str(e.value)), str(e.value)
    with pytest.raises(G.GuardError, match=r"control words not left zero: 1 bytes in 3 \.\. 3 of ctrl\[eval\]"):
        with G.guarded(0x00, guard_cpu=True):
            _bare(evaluation.DetectionEvaluator)._workspace(D, Gt)[3] = 1                                                       # the ticket


def test_sharing_a_control_workspace_is_limited_to_its_block():
    with G.guarded(0xFF, guard_cpu=True) as g:
        a = ops._ctrl_workspace(CPU, "rpn_conv_f32", 512)
        with g.sharing_ctrl("rpn_conv_f32"):
            b = ops._ctrl_workspace(CPU, "rpn_conv_f32", 512)
            assert ops._ctrl_workspace(CPU, "rpn_conv_f32", 512).data_ptr() == b.data_ptr() != a.data_ptr()
            assert ops._ctrl_workspace(CPU, "det_loss", 64).data_ptr() != ops._ctrl_workspace(CPU, "det_loss", 64).data_ptr()
        c = ops._ctrl_workspace(CPU, "rpn_conv_f32", 512)
        assert c.data_ptr() not in (a.data_ptr(), b.data_ptr()) and ops._ctrl_workspace(CPU, "rpn_conv_f32", 512).data_ptr() != c.data_ptr()


def hidden_buffers(x):
    keep, _ = [torch.empty((N,), dtype=torch.int64, device=x.device) for _ in range(2)]       # allocated in a comprehension: still this function's
    keep.copy_(torch.arange(N))
    return x[keep]                                      # a gather torch makes: the caller never sees `keep`


def test_buffers_behind_a_derived_result_are_asserted_to_be_arenas():
    with G.guarded(0xFF, guard_cpu=True) as g:
        hidden_buffers(g.place(_x()))
        g.expect_arenas("hidden_buffers", [(N,), (N,)])
        with pytest.raises(G.GuardError, match=r"no arena of shape \(37, 4\) was allocated in hidden_buffers"):
            g.expect_arenas("hidden_buffers", [(N,), (N, 4)])
        with pytest.raises(G.GuardError, match="no arena of shape"):
            g.expect_arenas("bypasses", [(N,)])
