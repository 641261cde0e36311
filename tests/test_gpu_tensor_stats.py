"""Per-tensor statistics on the GPU (csrc/telemetry.hip: frcnn_tensor_stats, through the C ABI and through optim.DeviceSGD /
telemetry.TensorStats).  Rows and state equal the numpy restatement (tests/tensor_stats_ref.py): finite sums on the bit patterns,
non-finite sums by class, maxima and counts exactly.  Rows, state and workspace are prefilled with 0xFF and have 0xFF behind them."""
import ctypes as C
import math
import struct

import numpy as np
import pytest
import torch

import grad_norm_ref as gn
import guarded
import tensor_stats_ref as ts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8
LENS = [0, 1, 3, 4, 5, 8191, 8192, 8193, 257 * 8192 - 3]                 # the last: 257 chunks, a finish thread takes a second trip
ROW = np.dtype([("g_sumsq", "<f8"), ("p_sumsq", "<f8"), ("m_sumsq", "<f8"), ("g_absmax", "<f4"), ("p_absmax", "<f4"),
                ("g_nonfinite", "<i4"), ("p_nonfinite", "<i4"), ("m_read", "<i4"), ("reserved", "<i4", (5,))])


def _place(values, offset):
    """A device buffer of 0xFF with `values` at `offset` floats past a 16-byte boundary; returns (buffer, address of the first value)."""
    n = values.size
    buf = np.full(PAD + 4 + n + PAD, 0xFFFFFFFF, np.uint32)
    buf[PAD + offset:PAD + offset + n] = values.view(np.uint32)
    dev = torch.from_numpy(buf.view(np.float32)).to(DEV)
    assert dev.data_ptr() % 16 == 0
    return dev, dev.data_ptr() + 4 * (PAD + offset)


class _Raw(object):
    """One SGD table over (g, p, m) lists of flat float32 arrays, stream s of tensor t at offs[s][t] floats past a 16-byte boundary."""

    def __init__(self, gs, ps, ms, born, offs):
        from faster_rcnn_pytorch_amd import _lib
        self.lib, self.n = _lib, len(gs)
        lens = [int(t.size) for t in gs]
        self.bufs = [[_place(t, o) for t, o in zip(stream, off)] for stream, off in zip((gs, ps, ms), offs)]
        self.before = [[b.clone() for b, _ in stream] for stream in self.bufs]
        ne = (C.c_int64 * self.n)(*lens)
        self.table_bytes = int(_lib.lib.frcnn_sgd_table_bytes(self.n, ne))
        host = np.zeros(self.table_bytes, np.uint8)
        nch = C.c_int32(0)
        vp = C.c_void_p * self.n
        g, p, m = ([a for _, a in stream] for stream in self.bufs)
        _lib.check(_lib.lib.frcnn_sgd_table_build_host(self.n, vp(*p), vp(*g), vp(*m), ne, (C.c_int32 * self.n)(*([0] * self.n)), 1,
                                                       host.ctypes.data_as(C.c_void_p), self.table_bytes, C.byref(nch)))
        self.n_chunks = nch.value
        assert self.n_chunks == sum(gn.n_chunks_of(n) for n in lens)
        self.table = torch.from_numpy(host).to(DEV)
        self.born = torch.tensor(list(born), dtype=torch.int32, device=DEV)
        self.ws_bytes = int(_lib.lib.frcnn_tensor_stats_workspace_bytes(self.n, self.n_chunks))
        assert self.ws_bytes >= 40 * self.n_chunks and self.ws_bytes % 16 == 0
        self.rows = torch.full((64 * self.n + 16,), 0xFF, dtype=torch.uint8, device=DEV)
        self.work = torch.full((self.ws_bytes + 16,), 0xFF, dtype=torch.uint8, device=DEV)
        self.state = None

    def set_state(self, every, tick=0, measured_tick=-1, measures=0, fg=-1, fp=-1):
        block = np.full(64 + 16, 0xFF, np.uint8)
        struct.pack_into("<iiiiii", block, 0, every, tick, measured_tick, measures, fg, fp)
        self.state = torch.from_numpy(block).to(DEV)

    def call(self, rows=None, ws_bytes=None):
        return self.lib.lib.frcnn_tensor_stats(
            C.c_void_p(self.table.data_ptr()), self.table_bytes, self.n, self.n_chunks, C.c_void_p(self.born.data_ptr()),
            C.c_void_p(self.rows.data_ptr() if rows is None else rows), C.c_void_p(self.state.data_ptr()), C.c_void_p(self.work.data_ptr()),
            self.ws_bytes if ws_bytes is None else ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def run(self):
        """One call; returns (rows as a structured array, the six state words), after checking what must not have been written."""
        self.lib.check(self.call(), "frcnn_tensor_stats")
        torch.cuda.synchronize()
        rows, state, work = self.rows.cpu().numpy(), self.state.cpu().numpy(), self.work.cpu().numpy()
        assert rows[64 * self.n:].tobytes() == b"\xff" * 16 and state[24:].tobytes() == b"\xff" * 56 and work[self.ws_bytes:].tobytes() == b"\xff" * 16
        for stream, before in zip(self.bufs, self.before):                 # g, p and m are only read
            for (b, _), was in zip(stream, before):
                assert torch.equal(b.view(torch.int32), was.view(torch.int32))
        self.work_host = work[:40 * self.n_chunks]
        return rows[:64 * self.n].view(ROW), struct.unpack("<iiiiii", state[:24].tobytes())

    def g_partials(self):
        return self.work_host[:8 * self.n_chunks].view(np.float64)

    def grad_norm_partials(self):
        wsb = int(self.lib.lib.frcnn_grad_norm_workspace_bytes(self.n_chunks))
        work = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
        state = torch.zeros(64, dtype=torch.uint8, device=DEV)
        self.lib.check(self.lib.lib.frcnn_grad_norm(C.c_void_p(self.table.data_ptr()), self.table_bytes, self.n, self.n_chunks, C.c_void_p(state.data_ptr()), None,
                                                    C.c_void_p(work.data_ptr()), wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return work.cpu().numpy()[:8 * self.n_chunks].view(np.float64)


def _bits(rows):
    return [ts.row_bits(r) for r in rows]


def _assert_rows(got, want, what=""):
    assert not got["reserved"].any()
    for t, (a, b) in enumerate(zip(_bits(got), _bits(want))):
        assert a == b, (what, t, a, b)


def _data(lens, seed, scale=0.02):
    rs = np.random.RandomState(seed)
    out = [[(rs.standard_normal(n) * s).astype(np.float32) for n in lens] for s in (scale, 1.0, 0.1)]
    for stream in out:
        for t in stream:
            t.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def lens_case():
    gs, ps, ms = _data(LENS, 41)
    born = [t % 2 for t in range(len(LENS))]
    ms = [m if b else np.full(m.size, np.nan, np.float32) for m, b in zip(ms, born)]          # an unborn momentum is NaN: it must not be loaded
    return gs, ps, ms, born, ts.rows_of(gs, ps, ms, born), np.concatenate([gn.chunk_partials(g)[0] for g in gs])


@pytest.mark.parametrize("offs", [0, 1, 2, 3, "mixed"], ids=lambda o: "off_%s" % o)
def test_c_abi_equals_the_restatement_at_every_alignment(lens_case, offs):
    gs, ps, ms, born, want, partials = lens_case
    n = len(gs)
    o = [[(3 * t + 1) % 4 for t in range(n)], [(t + 2) % 4 for t in range(n)], [t % 4 for t in range(n)]] if offs == "mixed" else [[offs] * n] * 3
    raw = _Raw(gs, ps, ms, born, o)
    raw.set_state(1, tick=5, measures=2)
    rows, state = raw.run()
    _assert_rows(rows, want, offs)
    assert state == (1, 6, 5, 3, -1, -1)
    assert [int(r["m_read"]) for r in rows] == [int(b and k > 0) for b, k in zip(born, LENS)] and all(r["m_sumsq"] == 0 for r, b in zip(rows, born) if not b)
    assert np.array_equal(raw.g_partials().view(np.uint64), partials.view(np.uint64)), "chunk partials vs the restatement"
    assert np.array_equal(raw.g_partials().view(np.uint64), raw.grad_norm_partials().view(np.uint64)), "chunk partials vs frcnn_grad_norm's workspace"


def test_three_hundred_one_element_tensors_and_the_first_non_finite_rows():
    rs = np.random.RandomState(42)
    mk = lambda: [v.reshape(1).copy() for v in (rs.standard_normal(300) * 3).astype(np.float32)]          # noqa: E731
    gs, ps, ms = mk(), mk(), mk()
    gs[270][0], gs[299][0], ps[257][0] = np.nan, np.inf, -np.inf           # behind row 255: the advance kernel's second trip finds them
    born = [1] * 300
    raw = _Raw(gs, ps, ms, born, [[t % 4 for t in range(300)], [(t + 1) % 4 for t in range(300)], [(t + 3) % 4 for t in range(300)]])
    assert raw.n_chunks == 300
    raw.set_state(1)
    rows, state = raw.run()
    _assert_rows(rows, ts.rows_of(gs, ps, ms, born))
    assert state == (1, 1, 0, 1, 270, 257)
    assert rows["g_nonfinite"].sum() == 2 and rows["p_nonfinite"].sum() == 1 and rows[299]["g_absmax"] == np.inf and rows[270]["g_absmax"] == 0


PLANT_LENS = [5, 8193, 257, 0, 1]
PLANTED = [("g", 0, 0, np.nan), ("g", 1, 8192, np.inf), ("p", 2, 100, -np.inf), ("m", 1, 5, np.nan), ("p", 4, 0, np.nan), ("m", 2, 256, np.inf),
           ("g", 2, 3, -np.inf)]


@pytest.fixture(scope="module")
def clean_case():
    gs, ps, ms = _data(PLANT_LENS, 43)
    offs = [[0, 0, 3, 0, 1], [1, 0, 0, 0, 2], [0, 2, 1, 0, 0]]
    raw = _Raw(gs, ps, ms, [1] * 5, offs)
    raw.set_state(1)
    rows, state = raw.run()
    _assert_rows(rows, ts.rows_of(gs, ps, ms, [1] * 5))
    assert state == (1, 1, 0, 1, -1, -1)
    return gs, ps, ms, offs, rows.copy()


@pytest.mark.parametrize("stream,tensor,index,value", PLANTED, ids=["%s%d_%s" % (s, t, v) for s, t, _, v in PLANTED])
def test_one_planted_non_finite_value_names_its_tensor_and_leaves_the_other_rows_alone(clean_case, stream, tensor, index, value):
    gs, ps, ms, offs, clean = clean_case
    data = {"g": [t.copy() for t in gs], "p": [t.copy() for t in ps], "m": [t.copy() for t in ms]}
    data[stream][tensor][index] = value
    raw = _Raw(data["g"], data["p"], data["m"], [1] * 5, offs)
    raw.set_state(1)
    rows, state = raw.run()
    want = ts.rows_of(data["g"], data["p"], data["m"], [1] * 5)
    _assert_rows(rows, want)
    assert state == (1, 1, 0, 1, tensor if stream == "g" else -1, tensor if stream == "p" else -1)
    for t in range(5):
        if t != tensor:
            assert rows[t].tobytes() == clean[t].tobytes(), ("a row that holds no planted value changed", t)
    r = rows[tensor]
    assert (int(r["g_nonfinite"]), int(r["p_nonfinite"])) == (int(stream == "g"), int(stream == "p"))
    s = r[stream + "_sumsq"]
    assert np.isnan(s) if np.isnan(value) else (np.isinf(s) and s > 0)
    if stream != "m":
        finite = np.abs(np.delete(data[stream][tensor], index))
        assert r[stream + "_absmax"] == (np.inf if np.isinf(value) else (finite.max() if finite.size else 0))         # a NaN never wins, an inf does


def test_every_three_over_seven_calls_and_a_foreign_state():
    lens = [3, 8193, 0]
    gs, ps, ms = _data(lens, 44)
    raw = _Raw(gs, ps, ms, [1, 0, 1], [[1, 0, 0], [0, 3, 0], [2, 0, 0]])
    ref = ts.State(3, 3)
    raw.set_state(3)
    gbuf, gaddr = raw.bufs[0][0]
    last = None
    for k in range(7):
        g0 = (gs[0] * np.float32(k + 1)).astype(np.float32)
        if k == 3:
            g0[1] = np.nan
        gbuf[PAD + 1:PAD + 4].copy_(torch.from_numpy(g0))
        raw.before[0][0] = gbuf.clone()
        measured = ref.call([g0, gs[1], gs[2]], ps, ms, [1, 0, 1])
        if k == 0:                                                        # before the first measuring call the rows are the caller's bytes
            assert measured
        rows, state = raw.run()
        assert state == ref.words(), k
        assert measured == (k in (0, 3, 6))
        if measured:
            _assert_rows(rows, ref.rows, k)
        else:
            assert rows.tobytes() == last, ("the rows changed on a tick that does not measure", k)
        last = rows.tobytes()
    assert ref.words() == (3, 7, 6, 3, -1, -1)
    for every, tick in ((0, 0), (-2, 4), (1, -1)):                         # a state block that is not ours: nothing is touched
        raw.rows.fill_(0xFF), raw.work.fill_(0xFF)
        raw.set_state(every, tick=tick, measured_tick=9, measures=9, fg=7, fp=7)
        raw.lib.check(raw.call())
        torch.cuda.synchronize()
        assert bool((raw.rows == 0xFF).all()) and bool((raw.work == 0xFF).all())
        assert struct.unpack("<iiiiii", raw.state.cpu().numpy()[:24].tobytes()) == (every, tick, 9, 9, 7, 7)


def test_c_abi_refusals_on_device_pointers_launch_nothing():
    gs, ps, ms = _data([5, 9000], 45)
    raw = _Raw(gs, ps, ms, [1, 1], [[0, 0]] * 3)
    raw.set_state(1)
    for kw, text in ((dict(rows=raw.rows.data_ptr() + 8), b"16-byte aligned"), (dict(ws_bytes=raw.ws_bytes - 1), b"short workspace"),
                     (dict(rows=raw.state.data_ptr()), b"overlap")):
        assert raw.call(**kw) != 0 and text in raw.lib.lib.frcnn_last_error(), kw
    torch.cuda.synchronize()
    assert bool((raw.rows == 0xFF).all()) and bool((raw.work == 0xFF).all())
    assert struct.unpack("<iiiiii", raw.state.cpu().numpy()[:24].tobytes()) == (1, 0, -1, 0, -1, -1)


# ---- through DeviceSGD ----------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 5), (64,), (17, 33), (1,), (9000,), (4, 3, 3, 3), (3 * 8192 + 5,)]
NAMES = ["t%d" % k for k in range(len(SHAPES))]


def _optimizer(seed=46, **kw):
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).to(DEV)) for s in SHAPES]
    grads = [torch.randn(*s, generator=gen) * 0.02 for s in SHAPES]
    for p, g in zip(params, grads):
        p.grad = g.to(DEV)
    return DeviceSGD(params, lr=2e-3, momentum=0.9, weight_decay=5e-4, **kw), params, grads


def _host(ts_):
    return [t.detach().cpu().numpy().reshape(-1).copy() for t in ts_]


def test_through_devicesgd_rows_names_and_the_sum_against_the_global_norm():
    opt, params, grads = _optimizer(max_grad_norm=1.0, tensor_stats=dict(names=NAMES, every=1))
    stats = opt.tensor_stats
    assert stats.rows_tensor.shape == (len(SHAPES), 64) and stats.state_tensor.shape == (64,) and stats.rows_tensor.is_cuda
    p0 = _host(params)
    opt.step()                                                            # measures BEFORE the update: the parameters of before, no momentum yet
    got = stats.read()
    want = ts.rows_of([g.numpy().reshape(-1) for g in grads], p0, [np.zeros(1)] * len(SHAPES), [0] * len(SHAPES))
    rows = stats.rows_tensor.cpu().numpy().reshape(-1).view(ROW)
    _assert_rows(rows, want, "first step")
    assert (got["every"], got["tick"], got["measured_tick"], got["measures"], got["first_nonfinite_g"], got["first_nonfinite_p"]) == (1, 1, 0, 1, None, None)
    for name, w in zip(NAMES, want):
        t = got["tensors"][name]
        assert t["grad_norm"] == math.sqrt(w["g_sumsq"]) and t["weight_norm"] == math.sqrt(w["p_sumsq"]) and t["momentum_norm"] == 0.0
        assert t["grad_absmax"] == float(w["g_absmax"]) and t["weight_absmax"] == float(w["p_absmax"]) and t["grad_nonfinite"] == t["weight_nonfinite"] == 0
    # the per-tensor sums against the global one: both are sums of the same non-negative squares, each within depth * 2^-53 of the exact
    # sum, so they differ by at most (D1 + D2) * 2^-53 relative; D1, D2 from the sizes alone, the sum over tensors formed exactly (fsum)
    numels = [int(np.prod(s)) for s in SHAPES]
    d1 = gn.additions_on_the_longest_path(numels)
    d2 = max(ts.additions_per_tensor(n) for n in numels) + 1
    total, glob = math.fsum(float(r["g_sumsq"]) for r in rows), opt.grad_stats()["sumsq"]
    print("sum of per-tensor g_sumsq %r, global sumsq %r, relative difference %.3e, bound %.3e" % (total, glob, abs(total - glob) / glob, (d1 + d2) * 2.0 ** -53))
    assert abs(total - glob) <= (d1 + d2) * 2.0 ** -53 * glob
    # second step: the momenta are born and read; a NaN in one gradient names its tensor although the step itself is not skipped
    p1, m1 = _host(params), _host([opt.state[p]["momentum_buffer"] for p in params])
    g2 = [g.numpy().reshape(-1).copy() for g in grads]
    g2[4][8999] = np.nan
    params[4].grad.view(-1)[8999] = float("nan")
    opt.step()
    got = stats.read()
    rows = stats.rows_tensor.cpu().numpy().reshape(-1).view(ROW)
    _assert_rows(rows, ts.rows_of(g2, p1, m1, [1] * len(SHAPES)), "second step")
    assert got["first_nonfinite_g"] == "t4" and got["first_nonfinite_g_index"] == 4 and got["tensors"]["t4"]["grad_nonfinite"] == 1
    assert all(t["momentum_read"] == 1 and t["momentum_norm"] > 0 for t in got["tensors"].values()) and got["measures"] == 2
    views = opt.scalar_views()
    assert sorted(views) == ["clip_coef", "grad_norm", "lr/0", "nonfinite", "skip"] and all(v.dim() == 0 and v.is_cuda for v in views.values())
    st = opt.grad_stats()
    assert float(views["lr/0"]) == float(np.float32(2e-3)) and int(views["nonfinite"]) == st["nonfinite"] == 1 and int(views["skip"]) == 0
    assert math.isnan(float(views["grad_norm"])) and math.isnan(float(views["clip_coef"]))


def test_every_is_carried_by_push_and_reset_starts_over():
    opt, params, grads = _optimizer(tensor_stats=True)
    stats = opt.tensor_stats
    assert stats.names == [str(k) for k in range(len(SHAPES))] and sorted(opt.scalar_views()) == ["lr/0"]
    stats.every = 2
    for _ in range(3):
        opt.step()                                                        # push_hyper() carries every = 2 in front of the first measure
    got = stats.read()
    assert (got["every"], got["tick"], got["measured_tick"], got["measures"]) == (2, 3, 2, 2)
    stats.measure()                                                       # on its own: tick 3 does not measure
    assert stats.read()["tick"] == 4 and stats.read()["measures"] == 2
    stats.reset()
    got = stats.read()
    assert (got["every"], got["tick"], got["measured_tick"], got["measures"]) == (2, 0, -1, 0) and got["tensors"]["0"]["grad_norm"] == 0.0
    for bad in (0, 1.5, True):
        stats.every = bad
        with pytest.raises(ValueError, match="every must be a Python int >= 1"):
            opt.step()
    stats.every = 2


def test_guard_bands_nothing_outside_rows_state_and_workspace_is_written():
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    gen = torch.Generator().manual_seed(47)
    shapes = [(5,), (8193,), (1,), (257,)]
    init = [torch.randn(*s, generator=gen).to(DEV) for s in shapes]
    grad = [torch.randn(*s, generator=gen).to(DEV) for s in shapes]

    def case(g):
        params = [torch.nn.Parameter(g.place(t)) for t in init]
        for p, t in zip(params, grad):
            p.grad = g.place(t)
        opt = DeviceSGD(params, lr=0.0, momentum=0.9, tensor_stats=True)   # momenta, table, rows | state and workspace come from arenas
        opt.prepare()
        opt.tensor_stats.measure()
        opt.tensor_stats.measure()
        stats = opt.tensor_stats
        return dict(block=stats._block, work=stats._work[:40 * stats._chunks], params=torch.cat([p.detach().reshape(-1) for p in params]),
                    grads=torch.cat([p.grad.reshape(-1) for p in params]))
    a, _ = guarded.run_both(case, derived=("params", "grads"))
    rows = a["block"].cpu().numpy()[64:].view(ROW)
    _assert_rows(rows, ts.rows_of(_host(grad), _host(init), [np.zeros(1)] * 4, [0] * 4))
    assert struct.unpack("<iiiiii", a["block"].cpu().numpy()[:24].tobytes()) == (1, 2, 1, 2, -1, -1)
    assert torch.equal(a["params"], torch.cat([t.reshape(-1) for t in init])) and torch.equal(a["grads"], torch.cat([t.reshape(-1) for t in grad]))
