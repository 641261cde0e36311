"""CPU-only checks of the device-side gradient accumulation (csrc/grad_accum.hip, optim.GradAccumulator, parallel.GraphStep(accumulate=)):

  * the numpy restatement (tests/grad_accum_ref.py) against windows worked by hand;
  * every refusal of the C ABI, with no device touched (the pointers are never dereferenced on the host);
  * GradAccumulator / GraphStep(accumulate=2) refusing CPU tensors and bad window values;
  * GraphStep(accumulate=1, graphs=False) on CPU tensors leaves the bits of a GraphStep built without the argument."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import grad_accum_ref as ga


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_restatement_follows_hand_worked_windows():
    """window 3, frame_skip 0,1,0 | 1,1,1 | 1,0,0 -- the state after every advance, written out."""
    st = ga.new_state(3)
    expect = [  # window phase live hold windows frames dropped
        [3, 1, 1, 1, 0, 1, 0], [3, 2, 1, 1, 0, 2, 1], [3, 0, 0, 0, 1, 3, 1],
        [3, 1, 0, 1, 1, 4, 2], [3, 2, 0, 1, 1, 5, 3], [3, 0, 0, 1, 2, 6, 4],
        [3, 1, 0, 1, 2, 7, 5], [3, 2, 1, 1, 2, 8, 5], [3, 0, 0, 0, 3, 9, 5]]
    for s, want in zip((0, 1, 0, 1, 1, 1, 1, 0, 0), expect):
        assert ga.words(ga.advance(st, s)) == want
    one = ga.new_state(1)                                                   # window 1: every live frame closes a window
    assert ga.words(ga.advance(one, 0)) == [1, 0, 0, 0, 1, 1, 0] and ga.words(ga.advance(one, 7)) == [1, 0, 0, 1, 2, 2, 1]
    bad = ga.new_state(0)                                                   # a block that is not ours is left alone
    assert ga.words(ga.advance(bad, 0)) == [0, 0, 0, 0, 0, 0, 0]


def test_restatement_table_and_rounding():
    nan = np.float32(np.nan)
    acc = [np.full(3, nan, np.float32)]
    st = ga.new_state(3)
    ga.accumulate(acc, [np.array([1.0, 2.0 ** 24, -0.0], np.float32)], st)              # p == 0, live: a copy, the NaN is not read
    assert ga.bits(acc[0]).tolist() == ga.bits(np.array([1.0, 2.0 ** 24, -0.0], np.float32)).tolist()
    ga.advance(st, 0)
    ga.accumulate(acc, [np.full(3, nan, np.float32)], st, frame_skip=1)                 # p > 0, left out: nothing is read or written
    assert acc[0].tolist() == [1.0, 2.0 ** 24, -0.0]
    ga.advance(st, 1)
    ga.accumulate(acc, [np.array([2.0 ** -24, 1.0, 0.0], np.float32)], st)              # p > 0, live: one rounding per add
    assert acc[0].tolist() == [1.0, 2.0 ** 24, 0.0]                                     # 1 + 2^-24 and 2^24 + 1 round to even; -0 + 0 = +0
    assert ga.bits(acc[0])[2] == 0
    ga.advance(st, 0)
    assert st["phase"] == 0 and st["hold"] == 0
    ga.accumulate(acc, [np.full(3, nan, np.float32)], st, frame_skip=5)                 # p == 0, left out: +0, neither is read
    assert ga.bits(acc[0]).tolist() == [0, 0, 0]
    st["phase"] = 3                                                                     # outside 0 .. window-1: nothing is touched
    ga.accumulate(acc, [np.ones(3, np.float32)], st)
    assert ga.bits(acc[0]).tolist() == [0, 0, 0]
    # in-order adds: (a + b) + c, not a + (b + c)
    a, b, c = np.float32(2.0 ** 24), np.float32(1.0), np.float32(1.0)
    acc, st = [np.zeros(1, np.float32)], ga.new_state(3)
    for v in (a, b, c):
        ga.accumulate(acc, [np.array([v])], st)
        ga.advance(st)
    assert acc[0][0] == 2.0 ** 24 and a + (b + c) != acc[0][0]


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def L():
    from faster_rcnn_pytorch_amd import _lib
    return _lib


def _arrays(srcs, accs, numels):
    n = len(numels)
    vp = C.c_void_p * n
    return vp(*srcs), vp(*accs), (C.c_int64 * n)(*numels)


def test_rows_per_launch_fits_the_argument_segment(L):
    R = L.lib.frcnn_grad_accum_rows_per_launch()
    assert 32 <= R and R * 28 + 64 <= 3072                                  # src, acc, numel, first chunk per row + the aligned bits


def test_accumulate_refuses_bad_arguments_before_touching_the_device(L):
    f = L.lib.frcnn_grad_accumulate
    S = C.c_void_p(0x7000)                                                  # never dereferenced on the host
    src, acc, num = _arrays([0x100000, 0x200000], [0x300000, 0x400000], [100, 200])
    ok = (2, src, acc, num, S, None, None)

    def refused(args, text):
        assert f(*args) == -1 and text.encode() in L.lib.frcnn_last_error() and b"grad_accumulate" in L.lib.frcnn_last_error(), (args, L.lib.frcnn_last_error())
    for k in (1, 2, 3, 4):                                                  # a NULL array or state
        refused(ok[:k] + (None,) + ok[k + 1:], "NULL argument")
    for n in (0, -1, 65537):
        refused((n,) + ok[1:], "n_tensors")
    refused(ok[:4] + (C.c_void_p(0x7008),) + ok[5:], "aligned")             # state not 16-byte aligned
    refused(ok[:5] + (C.c_void_p(0x8002),) + ok[6:], "aligned")             # frame_skip not 4-byte aligned
    for numels, text in (([100, -1], "negative size"), ([2 ** 40 + 1, 1], "too large")):
        refused((2,) + _arrays([0x100000, 0x200000], [0x300000, 0x400000], numels) + ok[4:], text)
    for srcs, accs, text in (([0, 0x200000], [0x300000, 0x400000], "NULL pointer"), ([0x100000, 0x200000], [0x300000, 0], "NULL pointer"),
                             ([0x100002, 0x200000], [0x300000, 0x400000], "not 4-byte aligned"),
                             ([0x100000, 0x200000], [0x300000, 0x400001], "not 4-byte aligned"),
                             ([0x100000, 0x200000], [0x300000, 0x300000 + 396], "overlapping acc"),     # the last word of row 0's acc
                             ([0x100000, 0x200000], [0x300000, 0x300000 - 796], "overlapping acc"),     # row 1 ends one word inside row 0
                             ([0x300000, 0x200000], [0x300000, 0x400000], "src of row 0 overlaps"),     # in place
                             ([0x100000, 0x300000 + 396], [0x300000, 0x400000], "src of row 1 overlaps"),
                             ([0x400000 - 396, 0x200000], [0x300000, 0x400000], "src of row 0 overlaps")):
        refused((2,) + _arrays(srcs, accs, [100, 200]) + ok[4:], text)
    # ranges that only touch do not overlap: 18 rows of 2^40 elements, every acc and every src beginning where the one before ends, pass the
    # overlap check and are refused by the one behind it (no accepted call may follow: it would launch on these made-up addresses)
    big, step = 2 ** 40, 2 ** 42
    refused((18,) + _arrays([0x1000 + (18 + t) * step for t in range(18)], [0x1000 + t * step for t in range(18)], [big] * 18) + ok[4:],
            "more than 2^31 - 1 chunks")
    refused((18,) + _arrays([0x1000 + (18 + t) * step - 4 for t in range(18)], [0x1000 + t * step for t in range(18)], [big] * 18) + ok[4:],
            "src of row 0 overlaps")                                        # the same, every src one element lower: its first is the last of an acc
    # the NULL and alignment checks come for empty rows too; overlap is about bytes, so an empty row overlaps nothing
    refused((2,) + _arrays([0, 0x200000], [0x300000, 0x400000], [0, 200]) + ok[4:], "NULL pointer")
    assert f(2, *_arrays([0x300000, 0x300000], [0x300000, 0x300000], [0, 0]), S, None, None) == 0      # every tensor empty: nothing is launched


def test_advance_refuses_bad_arguments_before_touching_the_device(L):
    f = L.lib.frcnn_grad_accum_advance
    for args, text in (((None, None, None), "NULL state"), ((C.c_void_p(0x7004), None, None), "aligned"),
                       ((C.c_void_p(0x7000), C.c_void_p(0x8001), None), "aligned")):
        assert f(*args) == -1 and text.encode() in L.lib.frcnn_last_error() and b"grad_accum_advance" in L.lib.frcnn_last_error()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_grad_accumulator_refuses_bad_windows_and_cpu(L):
    from faster_rcnn_pytorch_amd import optim
    for bad in (0, -1, 2.0, "2", None, True, torch.tensor(2)):
        with pytest.raises(ValueError, match="window"):
            optim.GradAccumulator(bad, "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.GradAccumulator(2, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.GradAccumulator(2, torch.device("cpu"), frame_skip=torch.zeros(1, dtype=torch.int32))
    assert struct.calcsize(optim.GA_STATE_FORMAT) == optim.GA_STATE_BYTES == 64
    assert optim.GA_STATE_KEYS == ga.KEYS and (optim.GA_OFF_PHASE, optim.GA_OFF_LIVE, optim.GA_OFF_HOLD, optim.GA_OFF_WINDOWS) == (4, 8, 12, 16)


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.trunk = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 16))
        self.rpn = torch.nn.Linear(16, 6)
        self.pool = torch.nn.Tanh()
        self.head = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4))

    def forward(self, x):
        f = self.trunk(x)
        r = self.rpn(f)
        return (r[:, :2], r[:, 2:], self.head(self.pool(f)))


def _tiny_step(**kw):
    from faster_rcnn_pytorch_amd import parallel
    torch.manual_seed(0)
    model = _Tiny()
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    xs = torch.arange(3 * 8, dtype=torch.float32).reshape(3, 8).sin()

    def forward_loss(f):
        a, b, c = pred = model(xs[f:f + 1])
        return (a.pow(2).mean() + b.abs().mean() + c.pow(2).mean(),), pred
    gs = parallel.GraphStep(model, opt, forward_loss, 3, torch.device("cpu"), cut_module=model.pool, late_modules=(model.head,), graphs=False, **kw)
    return model, opt, gs


def test_graph_step_accumulate_refuses_cpu_and_bad_values():
    for bad in (0, -2, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="accumulate"):
            _tiny_step(accumulate=bad)
    with pytest.raises(ValueError, match="HIP device"):
        _tiny_step(accumulate=2)
    with pytest.raises(ValueError, match="frame_skip"):
        _tiny_step(accumulate=1, frame_skip=torch.zeros(1, dtype=torch.int32))


def test_graph_step_accumulate_1_is_the_step_without_the_argument():
    """The no-change promise: five eager steps on CPU tensors, with accumulate=1 and without the argument -- parameters, momentum and the
    flat gradient buffers hold the same bits, no accumulator exists, and the report differs by the new key only."""
    ma, oa, ga_ = _tiny_step()
    mb, ob, gb = _tiny_step(accumulate=1)
    assert gb.accumulator is None and float(ga_.seed) == float(gb.seed) == 1.0
    for i in range(5):
        ga_.step(i)
        gb.step(i)
    for p, q in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
        assert torch.equal(oa.state[p]["momentum_buffer"].view(torch.int32), ob.state[q]["momentum_buffer"].view(torch.int32))
        assert torch.equal(p.grad.view(torch.int32), q.grad.view(torch.int32))
    ra, rb = ga_.report(), gb.report()
    assert rb.pop("accumulate") == 1 and ra.pop("accumulate") == 1 and ra == rb and rb["graphs"] == 0
