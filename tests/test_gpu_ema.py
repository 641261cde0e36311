"""The device-side weight average (csrc/ema.hip, the EMA instantiations of csrc/sgd.hip, optim.WeightEMA, DeviceSGD(ema=)) on the GPU.
Every comparison is on the bits (NaN by position) against tests/ema_ref.py -- which tests/test_ema_host.py pins to torch on the CPU --
or against tests/golden/ema.npz directly, unless a test says otherwise.

  1. seams: tensor sizes around the float4 tail and the 8192-element chunk, parameter and shadow independently at storage offsets of
     0-3 elements, special values at chunk edges, 12 updates under warm-up (both branches of the rule);
  2. the fused step equals a DeviceSGD step followed by update(): all four launch variants, two parameter groups;
  3. skipped steps (guard word, non-finite gradient, an all-empty accumulation window) move nothing, the next one continues the fixture;
  4. captured: the step with the average replayed under MultiStepLR equals the eager path, the fixture and torch on the CPU;
  5. swap: in place, an involution, capturable; updates while swapped are refused;
  6. guard bands (tests/guarded.py);
  7. a DetectGraph captured on the live weights evaluates the averaged ones inside applied();
  8. checkpoints."""
import copy

import numpy as np
import pytest
import torch

import ema_ref
import guarded
import sgd_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEAMS = [4095, 4096, 4097, 4100]                       # around one 16-byte sweep of 4096 elements; the dword sweep's 1023, 1024, 1025 stand below
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 8191, 8192, 8193, 2 * 8192 + 1025] + SEAMS + SEAMS
P_OFF = [0, 1, 2, 3, 0, 0, 1, 2, 3, 0, 0, 1] + [0, 0, 0, 0] + [0, 1, 0, 1]           # elements past a 16-byte boundary
E_OFF = [0, 0, 1, 2, 3, 1, 0, 3, 2, 2, 0, 1] + [0, 0, 0, 0] + [1, 0, 1, 0]           # index 4, 5, 9: the shadow misaligned under an aligned parameter; 10: both aligned; 11: both off by one
G_OFF = [0, 0, 2, 1, 3, 0, 2, 1, 3, 0, 0, 1] + [0, 0, 0, 0] + [0, 0, 0, 0]           # 12-15: every pointer of the row aligned; 16-19: exactly one off by one element
SPECIALS = [np.inf, -np.inf, np.nan, -0.0, 1e-40]
EDGES = (0, 8191, 8192, 2 * 8192 - 1, 2 * 8192)


@pytest.fixture(scope="module")
def z():
    return ema_ref.load()


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(sgd_ref.bits(a), sgd_ref.bits(b)) and np.array_equal(np.isnan(a), np.isnan(b))


def _host(ts):
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().copy() for t in ts]


def _view(values, off, place=None):
    """A view `off` elements into a fresh allocation that ends with the view (the slack in front holds 7.0: checked by _slack_untouched)."""
    base = torch.full((off + len(values),), 7.0, device=DEV)
    if place is not None:
        base = place(base)
    v = base[off:]
    v.copy_(torch.from_numpy(np.asarray(values, np.float32)))
    v._slack = base[:off]
    return v


def _slack_untouched(ts):
    return all(bool((t._slack == 7.0).all()) for t in ts)


def _with_specials(v, shift, every_edge=True):
    v = v.copy()
    pos = [i for i in EDGES + (len(v) - 1,) if 0 <= i < len(v)] if every_edge else [i for i in (0, len(v) - 1) if i >= 0 and len(v)]
    for j, i in enumerate(pos):
        v[i] = np.float32(SPECIALS[(j + shift) % len(SPECIALS)])
    return v


def _values(rs, sizes, scale=0.1):
    return [(rs.standard_normal(n) * scale).astype(np.float32) for n in sizes]


def _params(values, offs, place=None):
    return [_view(v, o, place).requires_grad_() for v, o in zip(values, offs)]


def _write(ts, values):
    with torch.no_grad():
        for t, v in zip(ts, values):
            t.copy_(torch.from_numpy(v))


# ------------------------------------------------------------------------------------------------------------------------ 1. seams
def test_update_at_the_seams_equals_the_restatement_for_twelve_updates_under_warmup():
    from faster_rcnn_pytorch_amd.optim import WeightEMA
    rs = np.random.RandomState(21)
    ps = _params(_values(rs, SIZES), P_OFF)
    es = [_view(np.zeros(n, np.float32), o) for n, o in zip(SIZES, E_OFF)]
    ema = WeightEMA(ps, decay=0.9998, warmup=True, shadow=es)
    assert all(_same(a, b) for a, b in zip(_host(es), _host(ps)))            # the shadows start as copies
    e_ref = [_with_specials(v, t, every_edge=False) for t, v in enumerate(_values(rs, SIZES))]
    _write(es, e_ref)
    st = ema_ref.State(0.9998, True)
    addr = [t.data_ptr() for t in ps + es]
    for k in range(12):
        p_now = _values(rs, SIZES)
        if k in (2, 5, 10):                                                  # 2 and 5: the large-weight branch; 10: the small one
            p_now = [_with_specials(v, t + k) for t, v in enumerate(p_now)]
        _write(ps, p_now)
        ema.update()
        e_ref = st.update(p_now, e_ref)
        got = _host(es)
        for t in range(len(SIZES)):
            assert _same(got[t], e_ref[t]), (k, SIZES[t])
        assert all(_same(a, b) for a, b in zip(_host(ps), p_now))            # the parameters are only read
    s = ema.stats()
    assert s == st.stats() and s["num_updates"] == 12 and s["w"] < 0.5
    assert addr == [t.data_ptr() for t in ps + es] and _slack_untouched(ps + es)


# ------------------------------------------------------------------------------------------------- 2. fused = two passes
VARIANTS = {"plain": {}, "clip": dict(max_grad_norm=0.05), "skip": dict(skip_nonfinite=True), "both": dict(max_grad_norm=0.05, skip_nonfinite=True)}
GROUP_HYPER = {"a": ((0.9, 5e-4), (0.0, 0.0)), "b": ((0.0, 5e-4), (0.9, 0.0))}


class _Set(object):
    """Parameters, gradients and shadows at the seam sizes and offsets, in two parameter groups, with a DeviceSGD and a WeightEMA."""

    def __init__(self, fused, variant, hyper, sizes=SIZES[1:], place=None):
        from faster_rcnn_pytorch_amd import optim
        rs = np.random.RandomState(22)
        self.ps = _params(_values(rs, sizes), P_OFF[1:], place)
        self.gs = [_view(np.zeros(s, np.float32), o, place) for s, o in zip(sizes, G_OFF[1:])]
        self.es = [_view(np.zeros(s, np.float32), o, place) for s, o in zip(sizes, E_OFF[1:])]
        for p, g in zip(self.ps, self.gs):
            p.grad = g
        groups = [dict(params=self.ps[i::2], lr=0.05 * (i + 1), momentum=hyper[i][0], weight_decay=hyper[i][1]) for i in range(2)]
        self.order = self.ps[0::2] + self.ps[1::2]                          # DeviceSGD's row order
        shadow = self.es[0::2] + self.es[1::2]
        self.guard = torch.zeros(1, dtype=torch.int32, device=DEV)
        gn = bool(VARIANTS[variant])
        if fused:
            self.ema = optim.WeightEMA(groups, decay=0.9, warmup=True, shadow=shadow)
            self.opt = optim.DeviceSGD(groups, guard=self.guard, ema=self.ema, **VARIANTS[variant])
        else:
            self.opt = optim.DeviceSGD(groups, guard=self.guard, **VARIANTS[variant])
            self.opt.prepare()                                               # allocates the gradient-norm state block
            word = self.opt._gn_state[optim.GN_OFF_SKIP:optim.GN_OFF_SKIP + 4].view(torch.int32) if gn else self.guard
            self.ema = optim.WeightEMA(groups, decay=0.9, warmup=True, shadow=shadow, guard=word)
        self.fused = fused

    def step(self):
        self.opt.step()
        if not self.fused:
            self.ema.update()

    def state(self):
        ms = [self.opt.state[p]["momentum_buffer"] for p in self.order]
        return dict(p=_host(self.order), m=_host(ms), e=_host(self.ema.shadow), born=self.opt.born(), ema=self.ema.stats())


@pytest.mark.parametrize("hyper", sorted(GROUP_HYPER))
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_fused_step_equals_device_sgd_step_then_update(variant, hyper):
    a, b = _Set(True, variant, GROUP_HYPER[hyper]), _Set(False, variant, GROUP_HYPER[hyper])
    al = lambda t: t.data_ptr() % 16 == 0   # noqa: E731
    assert al(a.ps[4]) and al(a.gs[4]) and al(a.opt.state[a.ps[4]]["momentum_buffer"]) and not al(a.es[4])      # only the shadow misaligned (1023)
    assert al(a.ps[8]) and al(a.gs[8]) and not al(a.es[8]) and al(a.ps[9]) and al(a.gs[9]) and al(a.es[9])       # 8192; 8193: the 16-byte path
    rs = np.random.RandomState(23)
    start = a.state()
    moved = []
    for k in range(5):
        grads = _values(rs, SIZES[1:], 0.02)
        guard = int(k == 1)
        if k == 3 and "skip_nonfinite" in VARIANTS[variant]:
            grads[6][100] = np.float32(np.inf)                               # a non-finite gradient: the step and the average stay
        for s in (a, b):
            _write(s.gs, grads)
            s.guard.fill_(guard)
            s.step()
        sa, sb = a.state(), b.state()
        for key in ("p", "m", "e"):
            for t, (x, y) in enumerate(zip(sa[key], sb[key])):
                assert _same(x, y), (k, key, t)
        assert sa["born"] == sb["born"] and sa["ema"] == sb["ema"], (k, sa["ema"], sb["ema"])
        moved.append(sa["ema"]["num_updates"])
    skipped = 1 + int("skip_nonfinite" in VARIANTS[variant])
    assert moved[0] == 1 and moved[1] == 1 and moved[-1] == 5 - skipped and sa["ema"]["skipped"] == skipped and sa["ema"]["refused"] == 0
    assert not _same(np.concatenate(sa["e"]), np.concatenate(start["e"])) and _slack_untouched(a.ps + a.gs + a.es)
    assert sa["born"] == [int(GROUP_HYPER[hyper][0][0] != 0)] * 10 + [int(GROUP_HYPER[hyper][1][0] != 0)] * 9


# ------------------------------------------------------------------------------------------------- 3. skipping, against the fixture
class _Mlp(object):
    """The fixture's 2-layer MLP on the GPU: DeviceSGD with the average fused in, MultiStepLR([4, 8]), gradients fed from the fixture."""

    def __init__(self, z, **kw):
        from faster_rcnn_pytorch_amd import optim
        self.z = z
        self.model = torch.nn.Sequential(torch.nn.Linear(7, 16), torch.nn.ReLU(), torch.nn.Linear(16, 3)).to(DEV)
        self.params = list(self.model.parameters())
        self.sizes = [p.numel() for p in self.params]
        assert [list(p.shape) for p in self.params] == [[d for d in s if d] for s in z["mlp_shapes"].tolist()]
        self.load_flat(self.params, z["mlp_p0"])
        for p in self.params:
            p.grad = torch.zeros_like(p)
        lr, mu, wd = (float(v) for v in z["mlp_hyper"])
        self.ema = optim.WeightEMA(self.params, decay=float(z["mlp_decay"]), warmup=False)
        self.opt = optim.DeviceSGD(self.params, lr=lr, momentum=mu, weight_decay=wd, ema=self.ema, **kw)
        self.sched = torch.optim.lr_scheduler.MultiStepLR(self.opt, milestones=[4, 8], gamma=0.1)

    def load_flat(self, ts, flat):
        off = 0
        with torch.no_grad():
            for t in ts:
                t.copy_(torch.from_numpy(np.ascontiguousarray(flat[off:off + t.numel()])).view_as(t))
                off += t.numel()

    def set_grads(self, flat):
        self.load_flat([p.grad for p in self.params], flat)

    def flat(self, ts):
        return np.concatenate([v.reshape(-1) for v in _host(ts)])

    def check(self, k, what=""):
        assert _same(self.flat(self.params), self.z["mlp_p"][k]), (what, k, "parameters")
        assert _same(self.flat(self.ema.shadow), self.z["mlp_e"][k]), (what, k, "average")


def test_skipped_steps_move_nothing_and_the_next_step_continues_the_fixture(z):
    guard = torch.zeros(1, dtype=torch.int32, device=DEV)
    run = _Mlp(z, guard=guard, skip_nonfinite=True)
    for k in range(12):
        assert run.opt.param_groups[0]["lr"] == z["mlp_lr"][k]
        if k in (3, 7):                                                      # a step that must not happen, in front of step k
            before = (run.flat(run.params), run.flat(run.ema.shadow), run.ema.stats()["num_updates"])
            bad = z["mlp_g"][k].copy()
            if k == 3:
                guard.fill_(1)
            else:
                bad[5] = np.float32(np.nan)
            run.set_grads(bad)
            run.opt.step()
            guard.fill_(0)
            assert _same(run.flat(run.params), before[0]) and _same(run.flat(run.ema.shadow), before[1])
            assert run.ema.stats()["num_updates"] == before[2] == k
        run.set_grads(z["mlp_g"][k])
        run.opt.step()
        run.sched.step()
        run.check(k)
    s = run.ema.stats()
    assert (s["num_updates"], s["skipped"], s["refused"], s["swapped"]) == (12, 2, 0, 0) and s["w"] == float(np.float32(1.0 - float(z["mlp_decay"])))
    assert run.opt.grad_stats()["skipped_steps"] == 2


def _graph_lr():
    import test_gpu_graph_lr as glr
    return glr


def test_accumulate_two_moves_the_average_once_per_closed_live_window():
    from faster_rcnn_pytorch_amd import optim, parallel
    glr = _graph_lr()
    model, frames = glr._mlp().to(DEV), glr._frames()
    params = list(model.parameters())
    empty = torch.zeros(1, dtype=torch.int32, device=DEV)

    def forward_loss(f):
        x, y = frames[f]
        out = model(x)
        return [torch.nn.functional.mse_loss(out, y)], (out, out)
    gs = parallel.GraphStep(model, None, forward_loss, 2, torch.device(DEV), accumulate=2, frame_skip=empty)
    ema = optim.WeightEMA(params, decay=0.9998, warmup=True)
    opt = optim.DeviceSGD(params, guard=gs.accumulator.hold, ema=ema, **glr.HYPER)
    gs.set_optimizer(opt)
    gs.capture()
    assert ema.stats()["num_updates"] == 2                                   # the warm-up: two windows per resident frame pair
    ema.reset()
    st = ema_ref.State(0.9998, True)
    e_ref = _host(params)
    assert ema.stats() == st.stats() and all(_same(a, b) for a, b in zip(_host(ema.shadow), e_ref))
    for i in range(8):
        empty.fill_(int(i in (4, 5)))                                        # the third window has no live frame
        p_before = _host(params)
        gs.step(i)
        p_now = _host(params)
        if i % 2 == 1 and i != 5:
            e_ref = st.update(p_now, e_ref)
            assert not all(_same(a, b) for a, b in zip(p_now, p_before))
        else:
            if i == 5:
                e_ref = st.update(p_now, e_ref, skip=1)
            assert all(_same(a, b) for a, b in zip(p_now, p_before))
        assert all(_same(a, b) for a, b in zip(_host(ema.shadow), e_ref)), i
        assert ema.stats() == st.stats(), i
    assert st.n == 3 and st.skipped == 1


# ------------------------------------------------------------------------------------------------------------------------ 4. graphs
def test_captured_step_with_the_average_replays_the_fixture_under_multisteplr(z):
    run, eager = _Mlp(z), _Mlp(z)
    run.set_grads(z["mlp_g"][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run.opt.step()                                                       # warm-up: builds both tables; moves weights and average
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run.opt.launch()
    torch.cuda.synchronize()
    assert run.ema.stats()["num_updates"] == 1                               # the capture ran nothing
    run.load_flat(run.params, z["mlp_p0"])                                   # back to the start, in place
    run.opt.load_state_dict(copy.deepcopy(eager.opt.state_dict()))
    run.ema.reset()
    assert run.ema.stats() == eager.ema.stats() and _same(run.flat(run.ema.shadow), z["mlp_p0"]) and run.opt.born() == [0] * 4
    for k in range(12):
        for r in (run, eager):
            r.set_grads(z["mlp_g"][k])
        run.opt.push_hyper()
        g.replay()
        eager.opt.step()
        run.sched.step(), eager.sched.step()
        run.check(k, "replay"), eager.check(k, "eager")
    assert run.ema.stats() == eager.ema.stats() and run.ema.stats()["num_updates"] == 12


def test_graphstep_u_carries_the_average_and_equals_eager_and_torch_on_the_cpu():
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from faster_rcnn_pytorch_amd import optim, parallel
    glr = _graph_lr()

    def make(graphs):
        model, frames = glr._mlp().to(DEV), glr._frames()
        params = list(model.parameters())
        ema = optim.WeightEMA(params, decay=0.9, warmup=False)
        opt = optim.DeviceSGD(params, ema=ema, **glr.HYPER)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[4, 8], gamma=0.1)

        def forward_loss(f):
            x, y = frames[f]
            out = model(x)
            return [torch.nn.functional.mse_loss(out, y)], (out, out)
        gs = parallel.GraphStep(model, opt, forward_loss, 2, torch.device(DEV), graphs=graphs)
        init, fresh = [p.detach().clone() for p in params], copy.deepcopy(opt.state_dict())
        gs.capture()
        with torch.no_grad():
            for p, s in zip(params, init):
                p.copy_(s)
        opt.load_state_dict(fresh)
        if graphs:
            assert gs.gU is not None and ema.stats()["num_updates"] == 2     # one warm-up step per resident frame
        ema.reset()                                                          # a clean average: a copy of the restored weights, n = 0
        assert ema.stats()["num_updates"] == 0 and all(torch.equal(e, p) for e, p in zip(ema.shadow, params))
        return model, params, ema, opt, sched, gs
    run, eager = make(True), make(False)
    twin = glr._mlp()
    topt = torch.optim.SGD(twin.parameters(), **glr.HYPER)
    tsched = torch.optim.lr_scheduler.MultiStepLR(topt, milestones=[4, 8], gamma=0.1)
    avg = AveragedModel(twin, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    avg.update_parameters(twin)                                              # its first call copies
    for i in range(12):
        run[5].step(i), eager[5].step(i)
        torch.cuda.synchronize()
        for p, q in zip(twin.parameters(), run[1]):
            p.grad = run[5].views[id(q)].detach().cpu().clone()
        topt.step()
        avg.update_parameters(twin)
        for r in (run, eager):
            r[4].step()
            r[3].push_hyper()
        tsched.step()
        want_p = [p.detach().numpy() for p in twin.parameters()]
        want_e = [p.detach().numpy() for p in avg.module.parameters()]
        for name, r in (("replay", run), ("eager", eager)):
            assert all(_same(a, b) for a, b in zip(_host(r[1]), want_p)), (name, i, "parameters")
            assert all(_same(a, b) for a, b in zip(_host(r[2].shadow), want_e)), (name, i, "average")
    assert run[2].stats()["num_updates"] == 12 and run[3].param_groups[0]["lr"] == pytest.approx(5e-4)


# ------------------------------------------------------------------------------------------------------------------------ 5. swap
def test_swap_is_in_place_an_involution_capturable_and_updates_while_swapped_are_refused():
    s = _Set(True, "plain", GROUP_HYPER["a"])
    rs = np.random.RandomState(24)
    _write(s.gs, _values(rs, SIZES[1:], 0.02))
    s.opt.step()                                                             # live and averaged weights differ now
    addr = [t.data_ptr() for t in s.ps + s.es]
    before = s.state()
    assert not _same(np.concatenate(before["p"]), np.concatenate(before["e"]))
    s.ema.swap()
    mid = s.state()
    assert all(_same(a, b) for a, b in zip(mid["p"], before["e"])) and all(_same(a, b) for a, b in zip(mid["e"], before["p"]))
    assert mid["ema"]["swapped"] == 1 and mid["ema"]["num_updates"] == 1
    # while the averaged weights are in: a fused step and an update() change nothing and are counted
    _write(s.gs, _values(rs, SIZES[1:], 0.02))
    s.opt.step()
    s.ema.update()
    held = s.state()
    for key in ("p", "m", "e"):
        assert all(_same(a, b) for a, b in zip(held[key], mid[key])), key
    assert held["born"] == mid["born"] and held["ema"] == dict(mid["ema"], refused=2)
    s.ema.swap()
    back = s.state()
    for key in ("p", "m", "e"):
        assert all(_same(a, b) for a, b in zip(back[key], before[key])), key
    assert back["ema"]["swapped"] == 0
    # captured: each replay is one swap
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.ema.swap()
    torch.cuda.synchronize()
    assert s.ema.stats()["swapped"] == 0                                     # the capture ran nothing
    g.replay()
    once = s.state()
    assert all(_same(a, b) for a, b in zip(once["p"], before["e"])) and once["ema"]["swapped"] == 1
    with s.ema.applied():                                                    # swapped in already: applied() swaps out and in again
        assert s.ema.stats()["swapped"] == 0
    g.replay()
    twice = s.state()
    assert all(_same(a, b) for a, b in zip(twice["p"], before["p"])) and all(_same(a, b) for a, b in zip(twice["e"], before["e"]))
    assert twice["ema"]["swapped"] == 0 and addr == [t.data_ptr() for t in s.ps + s.es] and _slack_untouched(s.ps + s.gs + s.es)
    s.opt.step()                                                             # and training goes on
    assert s.ema.stats()["num_updates"] == 2


def test_refusals_on_the_device():
    from faster_rcnn_pytorch_amd import optim
    p = torch.zeros(8, device=DEV).requires_grad_()
    q = torch.zeros(8, device=DEV).requires_grad_()
    with pytest.raises(TypeError, match="fp32 only"):
        optim.WeightEMA([torch.zeros(8, device=DEV, dtype=torch.float64).requires_grad_()])
    with pytest.raises(TypeError, match="not contiguous"):
        optim.WeightEMA([torch.zeros(16, device=DEV)[::2].requires_grad_()])
    with pytest.raises(ValueError, match="shadow tensors"):
        optim.WeightEMA([p, q], shadow=[torch.zeros(8, device=DEV)])
    with pytest.raises(RuntimeError, match="shape"):
        optim.WeightEMA([p], shadow=[torch.zeros(9, device=DEV)])
    with pytest.raises(optim._lib.FrcnnError, match="overlapping parameter and shadow"):
        optim.WeightEMA([p], shadow=[p.detach()]).update()
    ema = optim.WeightEMA([p, q], decay=0.5)
    with pytest.raises(AttributeError, match="fixed at construction"):
        ema.decay = 0.9
    with pytest.raises(ValueError, match="fixed at construction"):
        ema.load_state_dict(dict(ema.state_dict(), decay=0.9))
    for other in ([q, p], [p]):
        with pytest.raises(ValueError, match="exactly this optimizer's trainable parameters"):
            optim.DeviceSGD(other, lr=0.1, ema=ema)
    with pytest.raises(TypeError, match="must be a WeightEMA"):
        optim.DeviceSGD([p, q], lr=0.1, ema=object())
    assert optim.DeviceSGD([p, q], lr=0.1).ema is None
    with torch.no_grad():
        p.fill_(1.0)
        ema.reset()
        p.zero_()
        ema.copy_to()
    assert bool((p == 1.0).all()) and ema.stats()["num_updates"] == 0


# ------------------------------------------------------------------------------------------------------------------------ 6. guard bands
def test_update_fused_step_and_swap_write_nothing_outside_their_tensors():
    def case(g):
        s = _Set(True, "both", GROUP_HYPER["a"], place=g.place)
        rs = np.random.RandomState(25)
        for k in range(2):
            _write(s.gs, _values(rs, SIZES[1:], 0.02))
            s.opt.step()                                                     # the fused step (with the norm and the clip in front)
            s.ema.update()                                                   # the stand-alone update
        s.ema.swap()
        s.opt.step()                                                         # refused
        s.ema.swap()
        for t in [s.ema._state, s.ema._table, s.opt._born, s.opt._table] + [s.opt.state[p]["momentum_buffer"] for p in s.order]:
            assert g.arena_of(t) is not None
        assert _slack_untouched(s.ps + s.gs + s.es) and s.ema.stats()["num_updates"] == 4 and s.ema.stats()["refused"] == 1
        out = {"p%d" % i: t.detach() for i, t in enumerate(s.order)}
        out.update({"e%d" % i: t for i, t in enumerate(s.ema.shadow)})
        out.update({"m%d" % i: s.opt.state[p]["momentum_buffer"] for i, p in enumerate(s.order)})
        out["g_all"] = torch.cat(s.gs)                                       # the gradients are only read
        return out
    guarded.run_both(case, derived=("g_all",))


# ------------------------------------------------------------------------------------------------------------------------ 7. model level
def test_detect_graph_captured_on_the_live_weights_evaluates_the_averaged_ones_inside_applied():
    from faster_rcnn_pytorch_amd import optim
    from faster_rcnn_pytorch_amd.inference import DetectGraph
    from faster_rcnn_pytorch_amd.model import FRCNN
    H, W = 600, 1000

    def build():
        torch.manual_seed(0)
        return FRCNN(num_classes=21, sampling="host").to(DEV).eval()
    model = build()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():                                                    # as tests/test_gpu_detect.py: detections from random weights
        model.rpn.cls_layer.weight.mul_(30)
        model.rpn.reg_layer.weight.mul_(10)
        model.fast_rcnn_head.cls_head.weight.copy_(torch.randn(model.fast_rcnn_head.cls_head.weight.shape, generator=g) * 0.8)
        model.fast_rcnn_head.reg_head.weight.copy_(torch.randn(model.fast_rcnn_head.reg_head.weight.shape, generator=g) * 0.5)
    params = [p for p in model.parameters() if p.requires_grad]
    ema = optim.WeightEMA(params, decay=0.5, warmup=False)
    with torch.no_grad():                                                    # the live weights move on; one update pulls the average halfway
        model.fast_rcnn_head.cls_head.weight.mul_(1.5)
        model.fast_rcnn_head.reg_head.weight.mul_(0.5)
        model.rpn.reg_layer.weight.mul_(1.25)
    ema.update()
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(41)).to(DEV)
    dg = DetectGraph(model, (H, W), threshold=0.05)
    host = lambda det: [t.clone() for t in det.to_host()]   # noqa: E731
    equal = lambda a, b: len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))   # noqa: E731
    live = host(dg(x))
    addr = [p.data_ptr() for p in params]
    other = build()
    other.load_state_dict(ema.averaged_state_dict(model))
    want = host(other.detect(x, 0.05))
    with ema.applied():
        inside = host(dg(x))
    after = host(dg(x))
    assert len(live[1]) > 0 and len(want[1]) > 0 and not equal(live, want)
    assert equal(inside, want) and equal(after, live) and addr == [p.data_ptr() for p in params]
    assert ema.stats()["swapped"] == 0 and ema.stats()["num_updates"] == 1


# ------------------------------------------------------------------------------------------------------------------------ 8. checkpoints
def test_checkpoint_round_trip_continues_the_trajectory_and_files_without_ema_keep_their_keys(z, tmp_path):
    from faster_rcnn_pytorch_amd import checkpoint
    run = _Mlp(z)
    for k in range(6):
        run.set_grads(z["mlp_g"][k])
        run.opt.step()
        run.sched.step()
    with_ema = checkpoint.save_checkpoint(str(tmp_path / "a.pth.tar"), 5, run.model, run.opt, run.sched, ema=run.ema)
    without = checkpoint.save_checkpoint(str(tmp_path / "b.pth.tar"), 5, run.model, run.opt, run.sched)
    keys = ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert list(torch.load(without, weights_only=False)) == keys and list(torch.load(with_ema, weights_only=False)) == keys + ["ema_state_dict"]
    fresh = _Mlp(z)
    addr = [t.data_ptr() for t in fresh.ema.shadow]
    assert checkpoint.load_reference_checkpoint(fresh.model, with_ema, fresh.opt, fresh.sched, ema=fresh.ema) == 5
    assert addr == [t.data_ptr() for t in fresh.ema.shadow] and fresh.ema.stats() == run.ema.stats() and fresh.ema.stats()["num_updates"] == 6
    fresh.check(5, "loaded")
    for k in range(6, 12):
        fresh.set_grads(z["mlp_g"][k])
        fresh.opt.step()
        fresh.sched.step()
        fresh.check(k, "resumed")
    # a checkpoint without the key leaves the average at reset(): a copy of the loaded weights, n = 0
    plain = _Mlp(z)
    plain.set_grads(z["mlp_g"][0])
    plain.opt.step()
    checkpoint.load_reference_checkpoint(plain.model, without, plain.opt, plain.sched, ema=plain.ema)
    assert plain.ema.stats()["num_updates"] == 0 and _same(plain.flat(plain.ema.shadow), z["mlp_p"][5]) and _same(plain.flat(plain.params), z["mlp_p"][5])
    sd = run.ema.averaged_state_dict(run.model)
    assert list(sd) == list(run.model.state_dict()) and _same(np.concatenate([v.cpu().numpy().reshape(-1) for v in sd.values()]), z["mlp_e"][5])
