"""The device-side SGD on the GPU (csrc/sgd.hip through the C ABI and through optim.DeviceSGD).  No tolerance anywhere: parameters,
momentum and born words equal tests/golden/sgd.npz (torch.optim.SGD on the CPU) bit for bit, NaN by position; the numpy restatement
(tests/sgd_ref.py), checked here against the file's hashes once, supplies the arrays of the steps the file keeps as hashes only."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sgd_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8                                            # floats kept untouched between two tensors of a packed buffer
FILL = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def golden_cases():
    """[(case, p per step, m per step, born per step)]: computed once, read-only; every step's hash is the golden file's."""
    out = []
    for c in sgd_ref.load_cases(os.path.join(ROOT, "tests", "golden", "sgd.npz")):
        ps, ms, bs = sgd_ref.run_reference(c)
        for s in range(c.steps):
            assert sgd_ref.sha(ps[s]) == c.sha_p[s] and sgd_ref.sha(ms[s]) == c.sha_m[s] and np.array_equal(bs[s], c.born[s])
        for a in ps + ms + bs:
            a.setflags(write=False)
        out.append((c, ps, ms, bs))
    return out


def _same(a, b):
    return np.array_equal(sgd_ref.bits(a), sgd_ref.bits(b))


def _layout(lens, offset):
    """Start of every tensor in a packed buffer: 4-float aligned + `offset` floats, GUARD floats behind each; and the buffer's length."""
    starts, cur = [], GUARD
    for n in lens:
        cur = (cur + 3) // 4 * 4 + offset
        starts.append(cur)
        cur += int(n) + GUARD
    return starts, cur + 4


def _packed(values, lens, starts, total, case_off):
    buf = np.full(total, FILL, np.uint32)
    if values is not None:
        for t, n in enumerate(lens):
            buf[starts[t]:starts[t] + n] = values[case_off[t]:case_off[t + 1]].view(np.uint32)
    return torch.from_numpy(buf.view(np.float32)).to(DEV)


def _unpack(buf, lens, starts):
    a = buf.cpu().numpy()
    inside = np.zeros(a.size, bool)
    parts = []
    for t, n in enumerate(lens):
        inside[starts[t]:starts[t] + n] = True
        parts.append(a[starts[t]:starts[t] + n])
    return (np.concatenate(parts) if parts else a[:0]), a.view(np.uint32)[~inside]


def _run_abi(c, ps, ms, bs, offs):
    """All steps of one case through frcnn_sgd_table_build_host + frcnn_sgd_step, the tensors packed at storage offsets offs = (p, g, m)
    floats past a 16-byte boundary.  Checks every step; returns nothing."""
    from faster_rcnn_pytorch_amd import _lib
    T, G = len(c.lens), c.hyper.shape[1]
    lens = [int(n) for n in c.lens]
    lay = [_layout(lens, o) for o in offs]
    P = _packed(c.p0, lens, lay[0][0], lay[0][1], c.off)
    M = _packed(None, lens, lay[2][0], lay[2][1], c.off)                   # 0xFF everywhere: the first update must write, never read
    born = torch.zeros(T, dtype=torch.int32, device=DEV)
    hyper = torch.zeros(G, 4, dtype=torch.float32, device=DEV)
    ne = (C.c_int64 * T)(*lens)
    nbytes = int(_lib.lib.frcnn_sgd_table_bytes(T, ne))
    assert nbytes > 0
    table = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV)
    vp = C.c_void_p * T
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for s in range(c.steps):
        Gb = _packed(c.g[s], lens, lay[1][0], lay[1][1], c.off)
        host = np.zeros(nbytes, np.uint8)
        nch = C.c_int32(0)
        _lib.check(_lib.lib.frcnn_sgd_table_build_host(
            T, vp(*[P.data_ptr() + 4 * st for st in lay[0][0]]), vp(*[Gb.data_ptr() + 4 * st for st in lay[1][0]]),
            vp(*[M.data_ptr() + 4 * st for st in lay[2][0]]), ne, (C.c_int32 * T)(*[int(v) for v in c.group]), G,
            host.ctypes.data_as(C.c_void_p), nbytes, C.byref(nch)))
        assert nch.value == sum((n + 8191) // 8192 for n in lens)
        table[:nbytes].copy_(torch.from_numpy(host))
        h = np.zeros((G, 4), np.float32)
        h[:, :3] = c.hyper[s].astype(np.float32)
        h[:, 3] = np.nan                                                    # the unused slot is not read
        hyper.copy_(torch.from_numpy(h))
        _lib.check(_lib.lib.frcnn_sgd_step(C.c_void_p(table.data_ptr()), nbytes, T, nch.value, C.c_void_p(hyper.data_ptr()), G,
                                           C.c_void_p(born.data_ptr()), None, stream))
        torch.cuda.synchronize()
        p, p_guard = _unpack(P, lens, lay[0][0])
        m, m_guard = _unpack(M, lens, lay[2][0])
        assert _same(p, ps[s]), (c.name, offs, s, "parameters", int((sgd_ref.bits(p) != sgd_ref.bits(ps[s])).sum()))
        assert (p_guard == FILL).all() and (m_guard == FILL).all(), (c.name, offs, s, "a neighbour was written")
        b = born.cpu().numpy()
        assert np.array_equal(b, bs[s]), (c.name, offs, s, "born")
        for t in range(T):
            sl = c.span(t)
            if b[t]:
                assert _same(m[sl], ms[s][sl]), (c.name, offs, s, t, "momentum")
            else:
                assert (m[sl].view(np.uint32) == FILL).all(), (c.name, offs, s, t, "an unborn momentum was written")
        g_now, g_guard = _unpack(Gb, lens, lay[1][0])
        assert _same(g_now, c.g[s]) and (g_guard == FILL).all()           # the gradients are only read


@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 2, 3), (0, 0, 1)], ids=lambda o: "off%d%d%d" % o)
def test_c_abi_equals_golden_bit_for_bit_at_every_alignment(golden_cases, offs):
    for c, ps, ms, bs in golden_cases:
        _run_abi(c, ps, ms, bs, offs)


def _make_params(c, offset=0):
    """The case's tensors as Parameters that are views into one flat storage at `offset` floats past a 16-byte boundary."""
    lens = [int(n) for n in c.lens]
    starts, total = _layout(lens, offset)
    flat = _packed(c.p0, lens, starts, total, c.off)
    gflat = _packed(None, lens, starts, total, c.off)
    params = [torch.nn.Parameter(flat[starts[t]:starts[t] + n]) for t, n in enumerate(lens)]
    for t, p in enumerate(params):
        p.grad = gflat[starts[t]:starts[t] + lens[t]]
    return params, flat, gflat, lens, starts


def _groups(c, params, s=0):
    return [{"params": [p for t, p in enumerate(params) if c.group[t] == gi], "lr": float(c.hyper[s, gi, 0]), "momentum": float(c.hyper[s, gi, 1]),
             "weight_decay": float(c.hyper[s, gi, 2])} for gi in range(c.hyper.shape[1])]


@pytest.mark.parametrize("offset", [0, 1])
def test_device_sgd_equals_golden_bit_for_bit(golden_cases, offset):
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    for c, ps, ms, bs in golden_cases:
        params, flat, gflat, lens, starts = _make_params(c, offset)
        opt = DeviceSGD(_groups(c, params), lr=1.0)
        order = [t for gi in range(c.hyper.shape[1]) for t in range(len(lens)) if c.group[t] == gi]     # rows: group by group
        for p in params:
            opt.state[p]["momentum_buffer"].view(torch.int32).fill_(-1)   # 0xFF: the first update must write, never read
        addr = [opt.state[p]["momentum_buffer"].data_ptr() for p in params]
        for s in range(c.steps):
            for gi, pg in enumerate(opt.param_groups):
                pg["lr"], pg["momentum"], pg["weight_decay"] = (float(v) for v in c.hyper[s, gi])
            for t in range(len(lens)):
                gflat[starts[t]:starts[t] + lens[t]].copy_(torch.from_numpy(c.g[s, c.span(t)].copy()))
            opt.step()
            torch.cuda.synchronize()
            p, guard = _unpack(flat, lens, starts)
            assert _same(p, ps[s]), (c.name, offset, s)
            assert (guard == FILL).all()
            born = np.zeros(len(lens), np.int32)
            born[order] = opt.born()
            assert np.array_equal(born, bs[s])
            for t, q in enumerate(params):
                m = opt.state[q]["momentum_buffer"].cpu().numpy()
                if born[t]:
                    assert _same(m, ms[s][c.span(t)]), (c.name, offset, s, t)
                else:
                    assert (m.view(np.uint32) == FILL).all()
        assert addr == [opt.state[p]["momentum_buffer"].data_ptr() for p in params]
        sd = opt.state_dict()
        assert sorted(sd["state"]) == sorted(i for i, t in enumerate(order) if bs[-1][t])              # absent for unborn tensors


def _twin(shapes, seed, groups_of, steps, hyper_at, dev_kwargs=None):
    """DeviceSGD on the GPU and torch.optim.SGD on the CPU from the same random inputs; yields after every step."""
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) * 0.1 for s in shapes]
    grads = [[torch.randn(*s, generator=g) * 0.02 for s in shapes] for _ in range(steps)]
    cpu = [torch.nn.Parameter(t.clone()) for t in init]
    gpu = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    ref = torch.optim.SGD(groups_of(cpu), lr=1.0)
    mine = DeviceSGD(groups_of(gpu), lr=1.0, **(dev_kwargs or {}))
    return cpu, gpu, ref, mine, grads


def _set_grads(params, grads, device):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.clone().to(device)
        else:
            p.grad.copy_(g)


def _assert_twins_equal(cpu, gpu, ref, mine):
    torch.cuda.synchronize()
    for a, b in zip(cpu, gpu):
        assert _same(a.detach().numpy(), b.detach().cpu().numpy())
    sd_r, sd_m = ref.state_dict(), mine.state_dict()
    assert sorted(sd_r["state"]) == sorted(sd_m["state"])
    for i in sd_r["state"]:
        assert list(sd_r["state"][i]) == list(sd_m["state"][i]) == ["momentum_buffer"]
        assert _same(sd_r["state"][i]["momentum_buffer"].numpy(), sd_m["state"][i]["momentum_buffer"].cpu().numpy())
    assert [list(g) for g in sd_r["param_groups"]] == [list(g) for g in sd_m["param_groups"]]          # key for key, in order
    assert sd_r["param_groups"] == sd_m["param_groups"]


SHAPES = [(3, 5), (64,), (17, 33), (1,), (9000,), (4, 3, 3, 3)]


def _two_groups(ps):
    return [{"params": ps[:3], "lr": 2e-3, "momentum": 0.9, "weight_decay": 5e-4}, {"params": ps[3:], "lr": 1e-2, "momentum": 0.8, "weight_decay": 0.0}]


def test_five_steps_equal_torch_sgd_on_the_cpu_of_this_machine():
    cpu, gpu, ref, mine, grads = _twin(SHAPES, 1, _two_groups, 5, None)
    sched_r = torch.optim.lr_scheduler.MultiStepLR(ref, milestones=[2, 4], gamma=0.1)
    sched_m = torch.optim.lr_scheduler.MultiStepLR(mine, milestones=[2, 4], gamma=0.1)
    _assert_twins_equal(cpu, gpu, ref, mine)                                  # before any step: empty state on both sides
    for s in range(5):
        _set_grads(cpu, grads[s], "cpu"), _set_grads(gpu, grads[s], DEV)
        ref.step(), mine.step()
        sched_r.step(), sched_m.step()
        _assert_twins_equal(cpu, gpu, ref, mine)
    assert mine.param_groups[0]["lr"] == ref.param_groups[0]["lr"] != 2e-3


def test_eager_gradients_may_move_between_steps():
    cpu, gpu, ref, mine, grads = _twin(SHAPES, 2, _two_groups, 3, None)
    for s in range(3):
        ref.zero_grad(set_to_none=True), mine.zero_grad(set_to_none=True)      # new gradient tensors every step
        keep = [torch.empty(1000 * (s + 1), device=DEV)]                       # shifts what the allocator hands out
        _set_grads(cpu, grads[s], "cpu"), _set_grads(gpu, grads[s], DEV)
        ref.step(), mine.step()
        del keep
        _assert_twins_equal(cpu, gpu, ref, mine)


def test_guard_word_turns_the_step_into_a_no_op():
    guard = torch.zeros(1, dtype=torch.int32, device=DEV)
    cpu, gpu, ref, mine, grads = _twin(SHAPES, 3, _two_groups, 2, None, dict(guard=guard))
    for p in gpu:
        mine.state[p]["momentum_buffer"].view(torch.int32).fill_(-1)
    _set_grads(cpu, grads[0], "cpu"), _set_grads(gpu, grads[0], DEV)
    before = [p.detach().clone() for p in gpu]
    for skip in (1, -7):                                                      # before the first update: born words stay 0, momentum unwritten
        guard.fill_(skip)
        mine.step()
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32), b.detach().view(torch.int32)) for a, b in zip(before, gpu))
        assert all(bool((mine.state[p]["momentum_buffer"].view(torch.int32) == -1).all()) for p in gpu)
        assert mine.born() == [0] * len(gpu) and mine.state_dict()["state"] == {}
    guard.fill_(0)
    ref.step(), mine.step()                                                   # cleared: exactly ONE step has happened
    _assert_twins_equal(cpu, gpu, ref, mine)
    _set_grads(cpu, grads[1], "cpu"), _set_grads(gpu, grads[1], DEV)
    guard.fill_(1)                                                            # in the steady state: every byte as it was
    snap = [p.detach().clone() for p in gpu] + [mine.state[p]["momentum_buffer"].clone() for p in gpu]
    mine.step()
    torch.cuda.synchronize()
    now = [p.detach() for p in gpu] + [mine.state[p]["momentum_buffer"] for p in gpu]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(snap, now)) and mine.born() == [1] * len(gpu)
    guard.fill_(0)
    ref.step(), mine.step()
    _assert_twins_equal(cpu, gpu, ref, mine)


def test_checkpoints_round_trip_with_torch_sgd_both_ways_and_momentum_stays_in_place():
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    cpu, gpu, ref, mine, grads = _twin(SHAPES, 4, _two_groups, 6, None)
    for s in range(2):
        _set_grads(cpu, grads[s], "cpu"), _set_grads(gpu, grads[s], DEV)
        ref.step(), mine.step()
    _assert_twins_equal(cpu, gpu, ref, mine)
    # torch -> DeviceSGD: a FRESH DeviceSGD on the same weights takes torch's state (lr changed on the way: it travels in the groups)
    ref.param_groups[0]["lr"] = 7e-4
    fresh = DeviceSGD(_two_groups(gpu), lr=1.0)
    addr = [fresh.state[p]["momentum_buffer"].data_ptr() for p in gpu]
    fresh.load_state_dict(ref.state_dict())
    assert addr == [fresh.state[p]["momentum_buffer"].data_ptr() for p in gpu] and fresh.born() == [1] * len(gpu)
    assert fresh.param_groups[0]["lr"] == 7e-4
    for s in range(2, 4):
        _set_grads(cpu, grads[s], "cpu"), _set_grads(gpu, grads[s], DEV)
        ref.step(), fresh.step()
    _assert_twins_equal(cpu, gpu, ref, fresh)
    # DeviceSGD -> torch: a fresh torch optimizer on the CPU weights continues from DeviceSGD's state dict
    back = torch.optim.SGD(_two_groups(cpu), lr=1.0)
    back.load_state_dict({"state": {i: {"momentum_buffer": v["momentum_buffer"].cpu()} for i, v in fresh.state_dict()["state"].items()},
                          "param_groups": fresh.state_dict()["param_groups"]})
    for s in range(4, 6):
        _set_grads(cpu, grads[s], "cpu"), _set_grads(gpu, grads[s], DEV)
        back.step(), fresh.step()
    _assert_twins_equal(cpu, gpu, back, fresh)
    # an empty (never stepped) torch state dict un-bears every tensor: the next step is a first update again
    fresh.load_state_dict(torch.optim.SGD(_two_groups(cpu), lr=1.0).state_dict())
    assert fresh.born() == [0] * len(gpu) and addr == [fresh.state[p]["momentum_buffer"].data_ptr() for p in gpu]


def test_checkpoint_module_round_trips_device_sgd(tmp_path):
    from faster_rcnn_pytorch_amd import checkpoint
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3)).to(DEV)
    opt = DeviceSGD(net.parameters(), lr=2e-3, momentum=0.9, weight_decay=5e-4)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.1)
    net(torch.randn(4, 7, device=DEV)).sum().backward()
    opt.step(), sched.step()
    path = str(tmp_path / "ck.pth.tar")
    checkpoint.save_checkpoint(path, 0, net, opt, sched)
    want = [opt.state[p]["momentum_buffer"].clone() for p in net.parameters()]
    ref = torch.optim.SGD(net.parameters(), lr=2e-3, momentum=0.9, weight_decay=5e-4)         # the reference's optimizer reads the same file
    checkpoint.load_reference_checkpoint(net, path, ref, None, map_location=DEV)
    assert all(torch.equal(ref.state[p]["momentum_buffer"], w) for p, w in zip(net.parameters(), want)) and ref.param_groups[0]["lr"] == pytest.approx(2e-4)
    opt2 = DeviceSGD(net.parameters(), lr=2e-3, momentum=0.9, weight_decay=5e-4)
    checkpoint.load_reference_checkpoint(net, path, opt2, None, map_location="cpu")
    assert opt2.born() == [1] * 4 and all(torch.equal(opt2.state[p]["momentum_buffer"], w) for p, w in zip(net.parameters(), want))
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]


def test_refusals_through_python():
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    p = torch.nn.Parameter(torch.zeros(8, device=DEV))
    for kw, exc in ((dict(dampening=0.5), ValueError), (dict(nesterov=True, momentum=0.9), ValueError), (dict(maximize=True), ValueError)):
        with pytest.raises(exc, match="not supported"):
            DeviceSGD([p], lr=0.1, **kw)
    for bad in (torch.zeros(8, device=DEV, dtype=torch.float16), torch.zeros(8, device=DEV, dtype=torch.float64), torch.zeros(8, device=DEV, dtype=torch.bfloat16)):
        with pytest.raises(TypeError, match="fp32 only"):
            DeviceSGD([torch.nn.Parameter(bad)], lr=0.1)
    with pytest.raises(TypeError, match="not contiguous"):
        DeviceSGD([torch.nn.Parameter(torch.zeros(4, 6, device=DEV).t())], lr=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceSGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1)
    with pytest.raises(TypeError, match="guard"):
        DeviceSGD([p], lr=0.1, guard=torch.zeros(1, device=DEV))
    opt = DeviceSGD([p], lr=0.1, momentum=0.9)
    with pytest.raises(RuntimeError, match="has no gradient"):
        opt.step()                                                             # a trainable parameter whose .grad is None
    emb = torch.nn.Embedding(10, 4, sparse=True).to(DEV)
    opt_s = DeviceSGD(emb.parameters(), lr=0.1)
    emb(torch.tensor([1, 2], device=DEV)).sum().backward()
    with pytest.raises(TypeError, match="not a dense strided tensor"):
        opt_s.step()                                                           # a sparse gradient
    p.grad = torch.zeros(16, device=DEV)[::2]
    with pytest.raises(TypeError, match="not contiguous"):
        opt.step()
    p.grad = torch.zeros(8, device=DEV)
    for key, val in (("dampening", 0.1), ("nesterov", True), ("maximize", True)):  # changed behind the optimizer's back
        opt.param_groups[0][key] = val
        with pytest.raises(ValueError, match="not supported"):
            opt.step()
        opt.param_groups[0][key] = 0 if key == "dampening" else False
    opt.step()
    torch.cuda.synchronize()
    assert opt.born() == [1]


def test_refusals_through_the_c_abi_with_device_pointers():
    """The host-side refusals of tests/test_sgd_host.py again with real device addresses, and nothing launched by a refused step."""
    from faster_rcnn_pytorch_amd import _lib
    p, g, m = (torch.full((16,), float(v), device=DEV) for v in (1, 2, 3))
    born = torch.zeros(1, dtype=torch.int32, device=DEV)
    hyper = torch.tensor([[0.1, 0.9, 0.0, 0.0]], device=DEV)
    vp, ne, grp = C.c_void_p * 1, (C.c_int64 * 1)(16), (C.c_int32 * 1)(0)
    nbytes = int(_lib.lib.frcnn_sgd_table_bytes(1, ne))
    host = np.zeros(nbytes, np.uint8)
    nch = C.c_int32(0)

    def build(pp, gg, mm, numel=ne, group=grp, n_groups=1, size=nbytes):
        return _lib.lib.frcnn_sgd_table_build_host(1, vp(pp), vp(gg), vp(mm), numel, group, n_groups, host.ctypes.data_as(C.c_void_p), size, C.byref(nch))
    assert build(p.data_ptr(), g.data_ptr(), p.data_ptr() + 32) == -1 and b"overlapping parameter and momentum" in _lib.lib.frcnn_last_error()
    assert build(p.data_ptr(), g.data_ptr(), None) == -1 and b"NULL pointer in row 0" in _lib.lib.frcnn_last_error()
    assert build(p.data_ptr(), g.data_ptr(), m.data_ptr(), numel=(C.c_int64 * 1)(-16)) == -1 and b"negative size" in _lib.lib.frcnn_last_error()
    assert build(p.data_ptr(), g.data_ptr(), m.data_ptr(), group=(C.c_int32 * 1)(1)) == -1 and b"names group 1" in _lib.lib.frcnn_last_error()
    assert build(p.data_ptr(), g.data_ptr(), m.data_ptr(), size=nbytes - 1) == -3 and b"short table" in _lib.lib.frcnn_last_error()
    assert build(p.data_ptr(), g.data_ptr(), m.data_ptr()) == 0 and nch.value == 1
    table = torch.from_numpy(host).to(DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [C.c_void_p(table.data_ptr()), nbytes, 1, 1, C.c_void_p(hyper.data_ptr()), 1, C.c_void_p(born.data_ptr()), None, stream]
    for i, v, rc, text in ((1, nbytes - 1, -3, b"short table"), (0, None, -1, b"NULL pointer"), (4, None, -1, b"NULL pointer"), (6, None, -1, b"NULL pointer"),
                           (5, 0, -1, b"n_groups")):
        a = list(args)
        a[i] = v
        assert _lib.lib.frcnn_sgd_step(*a) == rc and text in _lib.lib.frcnn_last_error()
    torch.cuda.synchronize()
    assert bool((p == 1).all()) and bool((m == 3).all()) and int(born.item()) == 0
    _lib.check(_lib.lib.frcnn_sgd_step(*args))
    torch.cuda.synchronize()
    assert torch.equal(m, g) and int(born.item()) == 1 and torch.equal(p, torch.full((16,), 1.0, device=DEV) - torch.tensor(0.1, device=DEV) * 2)
