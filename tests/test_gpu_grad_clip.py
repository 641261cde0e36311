"""The device-side gradient norm, clipping and non-finite skip on the GPU (csrc/grad_norm.hip, sgd_update_kernel<true>, through the C ABI
and through optim.DeviceSGD).  No tolerance anywhere: sumsq, norm, coef and the counts equal the numpy restatement of the documented
summation order (tests/grad_norm_ref.py) bit for bit; the update, given the coefficient read back from the device, equals
torch.optim.SGD on the CPU fed with g.mul_(coef), NaN by position.  State block outputs and workspaces are prefilled with 0xFF."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import grad_norm_ref as gn
import sgd_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                                              # floats kept untouched around a tensor
LENS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 16385]
T = gn.FINISH_THREADS


def _place(values, offset):
    """A device buffer of 0xFF with `values` at `offset` floats past a 16-byte boundary; returns (buffer, view).  The view's address is
    buffer.data_ptr() + 4 * (PAD + offset), also for an empty view."""
    n = values.size
    buf = np.full(PAD + 4 + n + PAD, 0xFFFFFFFF, np.uint32)
    buf[PAD + offset:PAD + offset + n] = values.view(np.uint32)
    dev = torch.from_numpy(buf.view(np.float32)).to(DEV)
    assert dev.data_ptr() % 16 == 0
    return dev, dev[PAD + offset:PAD + offset + n]


class _Raw(object):
    """One table over `tensors` (numpy float32, flat) with gradient t at offs[t] floats past a 16-byte boundary; parameters and momenta
    are aligned placeholders that frcnn_grad_norm never touches."""

    def __init__(self, tensors, offs):
        from faster_rcnn_pytorch_amd import _lib
        self.lib, self.n = _lib, len(tensors)
        self.tensors = tensors
        lens = [int(t.size) for t in tensors]
        self.g = [_place(t, o) for t, o in zip(tensors, offs)]
        self.g_before = [b.clone() for b, _ in self.g]
        slots = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 + 4 for n in lens])])
        starts, total = slots[:-1], int(slots[-1])
        self.P, self.M = torch.zeros(total, device=DEV), torch.zeros(total, device=DEV)
        ne = (C.c_int64 * self.n)(*lens)
        self.table_bytes = int(_lib.lib.frcnn_sgd_table_bytes(self.n, ne))
        assert self.table_bytes > 0
        host = np.zeros(self.table_bytes, np.uint8)
        nch = C.c_int32(0)
        vp = C.c_void_p * self.n
        _lib.check(_lib.lib.frcnn_sgd_table_build_host(
            self.n, vp(*[self.P.data_ptr() + 4 * int(s) for s in starts]), vp(*[b.data_ptr() + 4 * (PAD + o) for (b, _), o in zip(self.g, offs)]),
            vp(*[self.M.data_ptr() + 4 * int(s) for s in starts]), ne, (C.c_int32 * self.n)(*([0] * self.n)), 1,
            host.ctypes.data_as(C.c_void_p), self.table_bytes, C.byref(nch)))
        self.n_chunks = nch.value
        assert self.n_chunks == sum(gn.n_chunks_of(n) for n in lens)
        self.table = torch.from_numpy(host).to(DEV)
        self.ws_bytes = int(_lib.lib.frcnn_grad_norm_workspace_bytes(self.n_chunks))
        assert self.ws_bytes >= 12 * self.n_chunks and self.ws_bytes % 16 == 0

    def run(self, max_norm, flags, guard=None, steps=7, skipped=2):
        """One frcnn_grad_norm; returns the state block as a dict of bit patterns / ints, checked for stray writes."""
        block = np.full(64, 0xFF, np.uint8)
        struct.pack_into("<fI", block, 0, max_norm, flags)
        struct.pack_into("<ii", block, 32, steps, skipped)
        state = torch.from_numpy(block).to(DEV)
        work = torch.full((self.ws_bytes + 16,), 0xFF, dtype=torch.uint8, device=DEV)
        gw = None if guard is None else torch.tensor([guard], dtype=torch.int32, device=DEV)
        self.lib.check(self.lib.lib.frcnn_grad_norm(
            C.c_void_p(self.table.data_ptr()), self.table_bytes, self.n, self.n_chunks, C.c_void_p(state.data_ptr()),
            None if gw is None else C.c_void_p(gw.data_ptr()), C.c_void_p(work.data_ptr()), self.ws_bytes,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        raw = bytes(state.cpu().numpy())
        mn, fl, sumsq, norm, coef, skip, nonfinite, st, sk = struct.unpack("<fIdffiiii24x", raw)
        assert struct.pack("<fI", mn, fl) == struct.pack("<fI", max_norm, flags) and raw[40:] == b"\xff" * 24       # inputs and reserved words as they were
        assert bytes(work[self.ws_bytes:].cpu().numpy()) == b"\xff" * 16                                             # nothing behind the workspace
        used = work[:12 * self.n_chunks].cpu().numpy()
        self.partials, self.counts = used[:8 * self.n_chunks].view(np.float64), used[8 * self.n_chunks:].view(np.int32)
        for (b, _), before in zip(self.g, self.g_before):                                                          # the gradients are only read
            assert torch.equal(b.view(torch.int32), before.view(torch.int32))
        return dict(sumsq=gn.f64_bits(sumsq), norm=gn.f32_bits(norm), coef=gn.f32_bits(coef), skip=skip, nonfinite=nonfinite, steps=st, skipped_steps=sk)


def _want(tensors, max_norm, flags, guard=None, steps=7, skipped=2):
    s = gn.state_after(tensors, max_norm, flags, guard, steps, skipped)
    return dict(s, sumsq=gn.f64_bits(s["sumsq"]), norm=gn.f32_bits(s["norm"]), coef=gn.f32_bits(s["coef"]))


@pytest.fixture(scope="module")
def lens_case():
    rs = np.random.RandomState(11)
    tensors = [(rs.standard_normal(n) * 0.02).astype(np.float32) for n in LENS]
    for t in tensors:
        t.setflags(write=False)
    want = _want(tensors, 0.25, gn.CLIP)
    parts = [gn.chunk_partials(t) for t in tensors]
    return tensors, want, np.concatenate([p for p, _ in parts])


@pytest.mark.parametrize("offs", [0, 1, 2, 3, "mixed"], ids=lambda o: "off_%s" % o)
def test_c_abi_equals_the_restatement_at_every_gradient_alignment(lens_case, offs):
    tensors, want, partials = lens_case
    o = [(3 * t + 1) % 4 for t in range(len(tensors))] if offs == "mixed" else [offs] * len(tensors)
    raw = _Raw(tensors, o)
    got = raw.run(0.25, gn.CLIP)
    assert np.array_equal(raw.partials.view(np.uint64), partials.view(np.uint64)), "chunk partials"
    assert not raw.counts.any()
    assert got == want, (got, want)                                       # the same bits as the aligned run: `want` does not know offsets
    assert np.float32(0) < np.array(want["coef"], np.uint32).view(np.float32) < np.float32(1)


@pytest.mark.parametrize("count", [1, T - 1, T, T + 1, 2 * T + 1])
def test_finish_kernel_trips_over_one_element_tensors(count):
    rs = np.random.RandomState(count)
    tensors = [v.reshape(1) for v in (rs.standard_normal(count) * 3).astype(np.float32)]
    raw = _Raw(tensors, [t % 4 for t in range(count)])
    assert raw.n_chunks == count
    assert raw.run(1.5, gn.CLIP | gn.SKIP_NONFINITE) == _want(tensors, 1.5, gn.CLIP | gn.SKIP_NONFINITE)


def test_one_tensor_of_123_chunks():
    rs = np.random.RandomState(3)
    x = (rs.standard_normal(1000003) * 0.01).astype(np.float32)
    for off in (0, 3):
        raw = _Raw([x], [off])
        assert raw.n_chunks == 123
        assert raw.run(1.0, gn.CLIP) == _want([x], 1.0, gn.CLIP), off


def test_exact_data_sums_exactly():
    """Integers times a power of two, the sum of the squares below 2^53 units: every partial sum is exact, so sumsq IS the integer sum."""
    rs = np.random.RandomState(4)
    ints = [rs.randint(-200, 201, n).astype(np.int64) for n in LENS + [40000]]
    exact = sum(int(v) * int(v) for t in ints for v in t)
    assert 0 < exact < 2 ** 53                                            # on the host side first
    scale = 2.0 ** -12
    tensors = [(t * scale).astype(np.float32) for t in ints]
    got = _Raw(tensors, [t % 4 for t in range(len(tensors))]).run(1.0, 0)
    assert got["sumsq"] == gn.f64_bits(exact * scale * scale) and got == _want(tensors, 1.0, 0)
    assert got["coef"] == gn.f32_bits(1.0)                                # clip off: exactly 1


def test_adverse_values_through_the_c_abi():
    both = gn.CLIP | gn.SKIP_NONFINITE
    huge = [np.full(20000, 3e38, np.float32), np.full(5, -3e38, np.float32)]
    got = _Raw(huge, [0, 1]).run(1.0, both)
    assert got == _want(huge, 1.0, both)
    assert np.isfinite(np.array(got["sumsq"]).view(np.float64)) and got["norm"] == gn.f32_bits(np.inf) and got["coef"] == gn.f32_bits(0.0)
    assert got["skip"] == 0 and got["nonfinite"] == 0                     # 3e38 is finite: nothing to skip
    rs = np.random.RandomState(6)
    sub = [(rs.randint(-(2 ** 23) + 1, 2 ** 23, n).astype(np.float64) * 2.0 ** -149).astype(np.float32) for n in (7, 300, 9000)]
    assert all((np.abs(t) < np.finfo(np.float32).tiny).all() for t in sub) and any(t.any() for t in sub)
    got = _Raw(sub, [0, 2, 1]).run(1e-30, both)
    assert got == _want(sub, 1e-30, both) and np.array(got["sumsq"]).view(np.float64) > 0
    zeros = [np.zeros(70, np.float32), -np.zeros(9000, np.float32), np.zeros(0, np.float32)]
    assert np.signbit(zeros[1]).all()
    got = _Raw(zeros, [0, 1, 0]).run(0.5, both)
    assert got == _want(zeros, 0.5, both) and got["sumsq"] == 0 and got["norm"] == 0 and got["coef"] == gn.f32_bits(1.0)
    empty = _Raw([np.zeros(0, np.float32)], [0])                           # no chunk at all: the finish kernel still runs
    assert empty.n_chunks == 0
    assert empty.run(0.5, both) == _want([np.zeros(0, np.float32)], 0.5, both)


def test_user_guard_and_counters_through_the_c_abi():
    x = [np.array([3.0, 4.0], np.float32)]
    raw = _Raw(x, [1])
    for flags in (0, gn.SKIP_NONFINITE, gn.CLIP | gn.SKIP_NONFINITE):
        for guard in (None, 0, 1, -5):
            assert raw.run(2.0, flags, guard, steps=40, skipped=9) == _want(x, 2.0, flags, guard, 40, 9), (flags, guard)
    got = raw.run(2.0, gn.CLIP, 1, steps=0, skipped=0)
    assert (got["norm"], got["skip"], got["steps"], got["skipped_steps"]) == (gn.f32_bits(5.0), 1, 1, 1)


# ---- through DeviceSGD, against torch.optim.SGD on the CPU -----------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(sgd_ref.bits(a), sgd_ref.bits(b))


class _Pair(object):
    """DeviceSGD on the GPU and torch.optim.SGD on the CPU from the same tensors.  Parameter t on the GPU is a view at p_offs[t] floats
    past a 16-byte boundary, its gradient one at g_offs[t]; momenta are prefilled with 0xFF (a first update writes, never reads)."""

    def __init__(self, shapes, seed, groups_of, p_offs, g_offs, **kw):
        from faster_rcnn_pytorch_amd.optim import DeviceSGD
        gen = torch.Generator().manual_seed(seed)
        self.gen, self.shapes = gen, shapes
        init = [torch.randn(*s, generator=gen) * 0.1 for s in shapes]
        self.cpu = [torch.nn.Parameter(t.clone()) for t in init]
        self.pbuf = [_place(t.numpy().reshape(-1), o) for t, o in zip(init, p_offs)]
        self.gbuf = [_place(np.zeros(t.numel(), np.float32), o) for t, o in zip(init, g_offs)]
        self.gpu = [torch.nn.Parameter(v.view(s)) for (_, v), s in zip(self.pbuf, shapes)]
        for p, (_, v), s in zip(self.gpu, self.gbuf, shapes):
            p.grad = v.view(s)
        self.ref = torch.optim.SGD(groups_of(self.cpu), lr=1.0)
        self.opt = DeviceSGD(groups_of(self.gpu), lr=1.0, **kw)
        for p in self.gpu:
            self.opt.state[p]["momentum_buffer"].view(torch.int32).fill_(-1)

    def grads(self, scale=0.02):
        return [torch.randn(*s, generator=self.gen) * scale for s in self.shapes]

    def set_grads(self, grads):
        for p, g in zip(self.gpu, grads):
            p.grad.copy_(g)

    def snapshot(self):
        torch.cuda.synchronize()
        return ([b.cpu().numpy().view(np.uint32).copy() for b, _ in self.pbuf] +
                [self.opt.state[p]["momentum_buffer"].cpu().numpy().view(np.uint32).copy() for p in self.gpu] + [np.array(self.opt.born())])

    def grad_bits(self):
        torch.cuda.synchronize()
        return [b.cpu().numpy().view(np.uint32).copy() for b, _ in self.gbuf]

    def twin_step(self, grads, coef):
        """What clip_grad_norm_ + optimizer.step() do on the CPU, with the coefficient the device derived."""
        for p, g in zip(self.cpu, grads):
            p.grad = g.clone()
            if coef is not None:
                p.grad.mul_(coef)
        self.ref.step()

    def assert_equal(self, what):
        torch.cuda.synchronize()
        born = self.opt.born()
        for k, (a, b) in enumerate(zip(self.cpu, self.gpu)):
            assert _same(a.detach().numpy(), b.detach().cpu().numpy()), (what, k, "parameter")
            m = self.opt.state[b]["momentum_buffer"].cpu().numpy()
            if "momentum_buffer" in self.ref.state.get(a, {}):
                assert born[k] == 1 and _same(self.ref.state[a]["momentum_buffer"].numpy(), m), (what, k, "momentum")
            else:
                assert born[k] == 0 and (m.view(np.uint32) == 0xFFFFFFFF).all(), (what, k, "an unborn momentum was written")
        for b, v in self.pbuf:                                            # nothing around a parameter was written
            a = b.cpu().numpy().view(np.uint32)
            assert (a[:PAD] == 0xFFFFFFFF).all() and (a[-PAD:] == 0xFFFFFFFF).all()


SHAPES = [(3, 5), (64,), (17, 33), (1,), (9000,), (4, 3, 3, 3)]
SEAMS = [(1023,), (1024,), (1025,), (4095,), (4096,), (4097,), (4100,)]      # around one dword sweep (1024) and one 16-byte sweep (4096) of the update


def _two_groups(ps):
    return [{"params": ps[:3], "lr": 2e-3, "momentum": 0.9, "weight_decay": 5e-4}, {"params": ps[3:], "lr": 1e-2, "momentum": 0.8, "weight_decay": 0.0}]


def _one_group(ps):
    return [{"params": ps, "lr": 2e-3, "momentum": 0.9, "weight_decay": 5e-4}]


def test_five_clipped_steps_two_groups_equal_torch_on_the_cpu_and_leave_the_gradients_alone():
    # the seam sizes once with every pointer of the row 16-byte aligned, once with exactly one of them off by one element
    pair = _Pair(SHAPES + SEAMS + SEAMS, 21, _two_groups, p_offs=[0, 1, 0, 2, 0, 3] + [0] * 7 + [1, 0, 1, 0, 1, 0, 1],
                 g_offs=[1, 0, 0, 3, 2, 0] + [0] * 7 + [0, 1, 0, 1, 0, 1, 0], max_grad_norm=5.0)
    coefs = []
    for s in range(5):
        if s == 3:
            pair.opt.max_grad_norm = 0.3                                  # between steps 2 and 3: push_hyper() (inside step()) carries it
        grads = pair.grads(0.02 if s != 1 else 0.2)
        pair.set_grads(grads)
        before = pair.grad_bits()
        pair.opt.step()
        st = pair.opt.grad_stats()
        want = gn.state_after([g.numpy() for g in grads], pair.opt.max_grad_norm, gn.CLIP, steps=s)
        assert gn.f64_bits(st["sumsq"]) == gn.f64_bits(want["sumsq"]) and gn.f32_bits(st["coef"]) == gn.f32_bits(want["coef"])
        assert (st["steps"], st["skipped_steps"], st["skip"], st["nonfinite"]) == (s + 1, 0, 0, 0) and st["max_norm"] == np.float32(pair.opt.max_grad_norm)
        assert float(pair.opt.grad_norm_tensor) == st["norm"] == float(want["norm"]) and pair.opt.grad_norm_tensor.dim() == 0
        pair.twin_step(grads, st["coef"])
        pair.assert_equal(s)
        assert all(np.array_equal(a, b) for a, b in zip(before, pair.grad_bits())), "p.grad was written"
        coefs.append(st["coef"])
    assert any(c == 1.0 for c in coefs[:3]) and all(0 < c < 1 for c in coefs[3:]) and any(c < 1.0 for c in coefs)
    sd = pair.opt.state_dict()                                            # torch.optim.SGD's, key for key: nothing of the clipping in it
    assert [list(g) for g in sd["param_groups"]] == [list(g) for g in pair.ref.state_dict()["param_groups"]]
    assert all(list(v) == ["momentum_buffer"] for v in sd["state"].values())


def test_norm_above_flt_max_moves_the_parameters_by_the_weight_decay_term_only():
    pair = _Pair([(20000,), (5,)], 22, _one_group, p_offs=[0, 1], g_offs=[0, 0], max_grad_norm=1.0, skip_nonfinite=True)
    grads = [torch.full((20000,), 3e38), torch.full((5,), -3e38)]
    pair.set_grads(grads)
    p0 = [p.detach().cpu().numpy().copy() for p in pair.gpu]
    pair.opt.step()
    st = pair.opt.grad_stats()
    assert np.isfinite(st["sumsq"]) and st["norm"] == np.inf and st["coef"] == 0.0 and st["skip"] == 0 and st["nonfinite"] == 0
    pair.twin_step(grads, st["coef"])
    pair.assert_equal("coef 0")
    for p, q in zip(p0, pair.gpu):                                        # g * 0 = +-0: d = wd * p, p' = fma(-lr, wd * p, p)
        d = sgd_ref.fma32(np.float32(5e-4), p, np.zeros_like(p))
        assert _same(sgd_ref.fma32(-np.float32(2e-3), d, p), q.detach().cpu().numpy()) and not _same(p, q.detach().cpu().numpy())


NONFINITE = [("nan_first_element", 0, 0, np.nan), ("nan_last_element_of_a_tail", 0, 4, np.nan), ("plus_inf_in_a_misaligned_tensor", 2, 100, np.inf),
             ("minus_inf_in_the_123_chunk_tensor", 1, 777777, -np.inf)]


@pytest.mark.parametrize("skip_on", [True, False], ids=["skip_on", "skip_off"])
@pytest.mark.parametrize("name,tensor,index,value", NONFINITE, ids=[c[0] for c in NONFINITE])
def test_one_non_finite_element(name, tensor, index, value, skip_on):
    shapes = [(5,), (1000003,), (257,)]
    pair = _Pair(shapes, 23, _one_group, p_offs=[0, 0, 0], g_offs=[0, 0, 3], max_grad_norm=0.5, skip_nonfinite=skip_on)
    clean = pair.grads()
    pair.set_grads(clean)
    pair.opt.step()                                                       # a clean step first: momenta born
    st = pair.opt.grad_stats()
    assert st["nonfinite"] == 0 and st["skip"] == 0 and 0 < st["coef"] < 1
    pair.twin_step(clean, st["coef"])
    pair.assert_equal("clean")
    planted = pair.grads()
    planted[tensor].view(-1)[index] = value
    pair.set_grads(planted)
    snap = pair.snapshot()
    pair.opt.step()
    st = pair.opt.grad_stats()
    assert st["nonfinite"] == 1 and st["steps"] == 2                      # the count equals what was planted
    assert np.isnan(st["coef"]) if np.isnan(value) else st["coef"] == 0.0
    if skip_on:
        assert st["skip"] == 1 and st["skipped_steps"] == 1
        assert all(np.array_equal(a, b) for a, b in zip(snap, pair.snapshot())), "a skipped step wrote something"
        again = pair.grads()
        pair.set_grads(again)
        pair.opt.step()                                                   # the next clean step is exactly one torch step
        st = pair.opt.grad_stats()
        assert (st["skip"], st["nonfinite"], st["steps"], st["skipped_steps"]) == (0, 0, 3, 1)
        pair.twin_step(again, st["coef"])
        pair.assert_equal("after the skipped step")
    else:
        assert st["skip"] == 0 and st["skipped_steps"] == 0
        pair.twin_step(planted, st["coef"])                               # the NaN spreads exactly as in the CPU twin
        pair.assert_equal("spread")
        assert bool(torch.isnan(pair.gpu[tensor]).any())


def test_skip_before_the_first_update_leaves_every_tensor_unborn():
    pair = _Pair(SHAPES, 24, _two_groups, p_offs=[0] * 6, g_offs=[0, 1, 2, 3, 0, 1], skip_nonfinite=True)
    bad = pair.grads()
    bad[4][8999] = float("inf")
    pair.set_grads(bad)
    snap = pair.snapshot()
    pair.opt.step()
    st = pair.opt.grad_stats()
    assert (st["skip"], st["nonfinite"], st["coef"], st["skipped_steps"]) == (1, 1, 1.0, 1) and pair.opt.born() == [0] * 6
    assert all(np.array_equal(a, b) for a, b in zip(snap, pair.snapshot())) and pair.opt.state_dict()["state"] == {}
    good = pair.grads()
    pair.set_grads(good)
    pair.opt.step()
    pair.twin_step(good, None)                                            # no clipping: the plain torch step
    pair.assert_equal("first real step")


def test_user_guard_together_with_skip_nonfinite():
    guard = torch.ones(1, dtype=torch.int32, device=DEV)
    pair = _Pair(SHAPES, 25, _two_groups, p_offs=[0] * 6, g_offs=[0] * 6, guard=guard, max_grad_norm=0.1, skip_nonfinite=True)
    grads = pair.grads()
    pair.set_grads(grads)
    snap = pair.snapshot()
    pair.opt.step()
    st = pair.opt.grad_stats()
    assert (st["skip"], st["nonfinite"], st["steps"], st["skipped_steps"]) == (1, 0, 1, 1) and 0 < st["coef"] < 1
    assert all(np.array_equal(a, b) for a, b in zip(snap, pair.snapshot()))
    guard.zero_()
    pair.opt.step()                                                       # cleared: exactly one step
    st = pair.opt.grad_stats()
    assert (st["skip"], st["steps"], st["skipped_steps"]) == (0, 2, 1)
    pair.twin_step(grads, st["coef"])
    pair.assert_equal("guard cleared")


def test_options_off_is_the_old_path_and_refusals_through_python():
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    p = torch.nn.Parameter(torch.zeros(8, device=DEV))
    p.grad = torch.ones(8, device=DEV)
    plain = DeviceSGD([p], lr=0.1)
    plain.step()
    assert plain._gn_state is None and plain._gn_work is None            # no new allocation, no state block
    with pytest.raises(RuntimeError, match="no gradient norm is measured"):
        plain.grad_stats()
    with pytest.raises(RuntimeError, match="no gradient norm is measured"):
        plain.grad_norm_tensor
    plain.max_grad_norm = 1.0
    with pytest.raises(ValueError, match="fixed there"):
        plain.step()
    for bad in (0, -2.0, float("nan"), torch.tensor(1.0, device=DEV)):
        with pytest.raises(ValueError, match="max_grad_norm"):
            DeviceSGD([p], lr=0.1, max_grad_norm=bad)
    with pytest.raises(ValueError, match="norm_type"):
        DeviceSGD([p], lr=0.1, max_grad_norm=1.0, norm_type=float("inf"))
    opt = DeviceSGD([p], lr=0.1, max_grad_norm=1.0)
    with pytest.raises(RuntimeError, match="first prepare"):
        opt.grad_stats()
    opt.step()
    addr = (opt._gn_state.data_ptr(), opt._gn_work.data_ptr())
    for bad, text in ((None, "cannot be switched off"), (0.0, "invalid max_grad_norm"), (torch.tensor(2.0), "got a tensor")):
        opt.max_grad_norm = bad
        with pytest.raises(ValueError, match=text):
            opt.step()
    opt.max_grad_norm = 4.0
    p.grad = torch.full((8,), 2.0, device=DEV)                            # a moved gradient: the table is rebuilt, the block stays
    opt.step()
    st = opt.grad_stats()
    assert addr == (opt._gn_state.data_ptr(), opt._gn_work.data_ptr()) and st["steps"] == 2 and st["max_norm"] == 4.0
    assert st["sumsq"] == 32.0 and st["coef"] == float(np.float32(4.0) / (np.float32(np.sqrt(32.0)) + np.float32(1e-6)))


def test_a_pending_max_grad_norm_is_refused_while_the_stream_is_capturing(monkeypatch):
    """The rule of the lr: the device block is written outside graphs.  (No capture is begun here: the check is the optimizer's own.)"""
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    p = torch.nn.Parameter(torch.ones(8, device=DEV))
    p.grad = torch.ones(8, device=DEV)
    opt = DeviceSGD([p], lr=0.1, max_grad_norm=1.0)
    opt.push_hyper(), opt.prepare()
    opt.max_grad_norm = 2.0                                                # not pushed
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="max_grad_norm changed and the stream is capturing"):
            opt.push_hyper()
    opt.step()                                                             # outside: carried; the step clips with 2.0
    st = opt.grad_stats()
    assert st["max_norm"] == 2.0 and st["steps"] == 1 and st["coef"] == float(np.float32(2.0) / (np.float32(np.sqrt(8.0)) + np.float32(1e-6)))
