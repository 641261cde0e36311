"""Device-side gradient accumulation (csrc/grad_accum.hip, optim.GradAccumulator, parallel.GraphStep(accumulate=)) on the GPU.  Every
comparison is on the int32 view of the bits.

  1. the op against the numpy restatement (tests/grad_accum_ref.py), inside guard-band arenas (tests/guarded.py);
  2. the same bits eager and captured;
  3. with DeviceSGD(guard=acc.hold) against torch.optim.SGD on the CPU, plain and with clipping + the non-finite skip;
  4. both model mirrors: one captured graph set with accumulate=2 against eager accumulation into .grad;
  5. two ranks on one GPU over gloo against a single-process run."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import grad_accum_ref as ga
import grad_norm_ref as gn
import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIPS = (0, 1, 0, 7, 1, -1, 1, 0, 0)                                        # window 3: 0,1,0 | 1,1,1 | 1,0,0 (any non-zero word skips)
PLACEMENTS = {"aligned": (0, 0), "acc+1": (1, 0), "src+2": (0, 2)}          # element offsets of (acc, src) from a 512-byte boundary
SENTINEL = -12345.5


def _sizes():
    from faster_rcnn_pytorch_amd import _lib
    R = int(_lib.lib.frcnn_grad_accum_rows_per_launch())
    seams = [1023, 1024, 1025, 4095, 4096, 4097, 4100]                      # around one dword sweep (1024) and one 16-byte sweep (4096)
    return [0, 1, 3, 4, 5] + seams + [8191, 8192, 8193, 2 * 8192 + 5] + [7] * (R + 1)     # the R + 1 small ones cross a launch boundary


def _sources(sizes):
    """Per frame, per tensor: float32 arrays.  Skipped frames carry NaN and inf only."""
    rs = np.random.RandomState(11)
    out = []
    for f, s in enumerate(SKIPS):
        if s != 0:
            out.append([np.full(n, (np.nan, np.inf, -np.inf)[(f + k) % 3], np.float32) for k, n in enumerate(sizes)])
        else:
            out.append([(rs.standard_normal(n) * 10.0 ** rs.randint(-3, 4)).astype(np.float32) for n in sizes])
    return out


def _reference(sizes, sources):
    """The restatement over the nine frames: (accumulators after each accumulate, state words after each advance)."""
    st = ga.new_state(3)
    accs = [np.full(n, np.nan, np.float32) for n in sizes]
    snaps, states = [], []
    for f, s in enumerate(SKIPS):
        if f % 3 == 0:
            for a in accs:
                a[...] = np.nan
        ga.accumulate(accs, sources[f], st, s)
        snaps.append(np.concatenate(accs).view(np.int32).copy())
        states.append(ga.words(ga.advance(st, s)))
    return snaps, states


class _Case(object):
    """Accumulators, sources, frame_skip word and state block of one placement, each between guards when `g` is a guarded context."""

    def __init__(self, g, placement, sizes, halves=False):
        from faster_rcnn_pytorch_amd import optim
        dev = torch.device(DEV)
        oa, os_ = PLACEMENTS[placement]
        self.sizes, self.halves = sizes, halves
        self.acc_base = [torch.full((n + oa,), SENTINEL, device=dev) for n in sizes]        # under `g`, torch.full & co. hand out arenas
        self.src_base = [torch.full((n + os_,), SENTINEL, device=dev) for n in sizes]
        self.accs = [b[oa:] for b in self.acc_base]
        self.srcs = [b[os_:] for b in self.src_base]
        self.lead = [b[:oa] for b in self.acc_base]                         # the elements in front of a shifted accumulator: not a guard's
        self.skip = torch.zeros(1, dtype=torch.int32, device=dev)
        self.acc = optim.GradAccumulator(3, dev, frame_skip=self.skip)      # its state block comes from torch.zeros: an arena under `g`
        self.stage = torch.empty(sum(sizes), device=dev)

    def load(self, f, sources):
        if f % 3 == 0:                                                      # NaN before every window: never read at phase 0
            self.stage.fill_(float("nan"))
            pairs = [(d, s) for d, s in zip(self.accs, self.stage.split(self.sizes)) if d.numel()]
            torch._foreach_copy_([d for d, _ in pairs], [s for _, s in pairs])
        self.stage.copy_(torch.from_numpy(np.concatenate(sources[f])))
        pairs = [(d, s) for d, s in zip(self.srcs, self.stage.split(self.sizes)) if d.numel()]
        torch._foreach_copy_([d for d, _ in pairs], [s for _, s in pairs])
        self.skip.fill_(SKIPS[f])

    def launch(self):
        if self.halves:                                                     # two calls that must see the same phase, then the bookkeeping
            h = len(self.accs) // 2
            self.acc.accumulate(self.accs[:h], self.srcs[:h])
            self.acc.accumulate(self.accs[h:], self.srcs[h:])
        else:
            self.acc.accumulate(self.accs, self.srcs)

    def bits(self):
        return torch.cat([a.reshape(-1) for a in self.accs]).view(torch.int32).cpu().numpy()

    def state_words(self):
        return self.acc._state.view(torch.int32).cpu().tolist()

    def untouched(self):
        """The elements in front of every shifted accumulator, and the sources as they were loaded last."""
        lead = torch.cat([l for l in self.lead] + [torch.full((1,), SENTINEL, device=self.stage.device)])
        srcs = torch.cat([s.reshape(-1) for s in self.srcs])
        return bool((lead == SENTINEL).all()) and torch.equal(srcs.view(torch.int32), self.stage.view(torch.int32))


def _eager(g, placement, sizes, sources, frames, halves=False):
    """Eager calls over the first `frames` frames; asserts against the restatement after every call and every advance."""
    snaps, states = _reference(sizes, sources)
    c = _Case(g, placement, sizes, halves)
    holds = []
    for f in range(frames):
        c.load(f, sources)
        c.launch()
        got = c.bits()
        assert np.array_equal(got, snaps[f]), "frame %d (%s): %d elements differ, first at %d" % (
            f, placement, int((got != snaps[f]).sum()), int(np.nonzero(got != snaps[f])[0][0]))
        c.acc.advance()
        words = c.state_words()
        assert words[:7] == states[f] and words[7:] == [0] * 9, (f, words)
        assert c.acc.stats() == dict(zip(ga.KEYS, states[f]))
        holds.append(int(c.acc.hold.item()))
        assert c.acc.closing == (f % 3 == 1)                                # the host mirror follows
    assert c.untouched()
    return c, holds, snaps


@pytest.mark.parametrize("placement", sorted(PLACEMENTS))
def test_op_equals_the_restatement_inside_guard_bands(placement):
    sizes = _sizes()
    sources = _sources(sizes)

    def case(g):
        c, holds, _ = _eager(g, placement, sizes, sources, len(SKIPS))
        assert [i + 1 for i, h in enumerate(holds) if h == 0] == [3, 9]     # hold is 0 exactly after frames 3 and 9
        assert g.arena_of(c.acc._state) is not None
        return {"acc%d" % k: a for k, a in enumerate(c.accs)}
    guarded.run_both(case)


def test_same_bits_eager_and_captured():
    """One graph: two accumulate calls and one advance; six replays over the first two windows, sources refilled before each."""
    sizes = _sizes()
    sources = _sources(sizes)
    _, _, snaps = _eager(None, "acc+1", sizes, sources, 6, halves=True)     # the eager calls (checked against the restatement on the way)
    c = _Case(None, "acc+1", sizes, halves=True)
    c.load(0, sources)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.launch()
        c.acc.advance()
    assert c.acc.stats()["frames"] == 0 and not c.acc.closing               # a capture runs nothing, and the mirror has not moved
    holds = []
    for f in range(6):
        c.load(f, sources)
        graph.replay()
        c.acc.tick()
        assert np.array_equal(c.bits(), snaps[f]), f
        holds.append(int(c.acc.hold.item()))
    assert holds == [1, 1, 0, 1, 1, 1] and c.acc.stats() == dict(window=3, phase=0, live=0, hold=1, windows=2, frames=6, dropped=4)
    spare = torch.zeros(4, device=DEV)
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        spare.add_(1.0)
        with pytest.raises(RuntimeError, match="outside graphs"):
            c.acc.reset_window()
    c.acc.advance()
    c.acc.reset_window()
    assert c.acc.stats()["phase"] == 0 and c.acc.stats()["frames"] == 7 and not c.acc.closing
    with pytest.raises(TypeError, match="fp32"):
        c.acc.accumulate([c.accs[3].double()], [c.srcs[3].double()])
    with pytest.raises(RuntimeError, match="shape"):
        c.acc.accumulate([c.accs[3]], [c.srcs[4]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c.acc.accumulate([c.accs[3].cpu()], [c.srcs[3]])


# ------------------------------------------------------------------------------------------------ 3. with DeviceSGD(guard=acc.hold)
SHAPES = [(37,), (5, 11), (8200,), (1,), (3, 4, 5)]


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("skips", [(0, 0, 1, 1, 1, 0), (1, 1, 0, 0, 0, 1)])
def test_device_sgd_steps_once_per_live_window(clip, skips):
    """K = 2, three windows, one of them all-skipped (the middle one; in the second pattern the FIRST, so that born words are still 0), a
    step attempted after every frame.  torch.optim.SGD on the CPU gets g0 then grad.add_(g1) and steps once per live window."""
    from faster_rcnn_pytorch_amd import optim
    dev = torch.device(DEV)
    lr, mu, wd = 2e-3, 0.9, 5e-4
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(*s, generator=gen) * 0.1 for s in SHAPES]
    frames = [[torch.randn(*s, generator=gen) * 0.02 for s in SHAPES] for _ in skips]
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if clip else {}
    # the device
    skip = torch.zeros(1, dtype=torch.int32, device=dev)
    acc = optim.GradAccumulator(2, dev, frame_skip=skip)
    ps = [torch.nn.Parameter(t.to(dev)) for t in init]
    for p in ps:
        p.grad = torch.full_like(p, float("nan"))                           # the accumulators: written by every window's first frame
    opt = optim.DeviceSGD(ps, lr=lr, momentum=mu, weight_decay=wd, guard=acc.hold, **kw)
    # torch on the CPU
    cps = [torch.nn.Parameter(t.clone()) for t in init]
    copt = torch.optim.SGD(cps, lr=lr, momentum=mu, weight_decay=wd)

    def state():
        return [p.detach().cpu() for p in ps] + [opt.state[p]["momentum_buffer"].cpu() for p in ps], opt.born()

    def cpu_state():
        return [p.detach().clone() for p in cps] + [copt.state[p]["momentum_buffer"].clone() if "momentum_buffer" in copt.state[p] else torch.zeros_like(p)
                                                   for p in cps]
    live = 0
    for f, s in enumerate(skips):
        before = state()
        skip.fill_(s)
        bad = float("nan") if f % 2 else float("inf")
        acc.accumulate([p.grad for p in ps], [torch.full_like(p, bad) if s else g.to(dev) for p, g in zip(ps, frames[f])])
        acc.advance()
        opt.step()
        if s == 0:
            for p, g in zip(cps, frames[f]):
                if live == 0:
                    p.grad = torch.zeros_like(p).add_(g) if f % 2 else g.clone()     # behind a skipped first frame the sum starts from +0
                else:
                    p.grad.add_(g)
            live += 1
        closed = f % 2 == 1
        if closed and live:
            if clip:
                st = gn.state_after([p.grad.numpy().reshape(-1) for p in cps], 1.0, gn.CLIP | gn.SKIP_NONFINITE)
                got = opt.grad_stats()
                assert gn.f32_bits(got["norm"]) == gn.f32_bits(st["norm"]) and got["skip"] == 0 and got["nonfinite"] == 0, (f, got, st)
                for p in cps:
                    p.grad.mul_(torch.tensor(st["coef"]))
            copt.step()
        if closed:
            live = 0
        after = state()
        if closed and int(acc.hold.item()) == 0:
            want = cpu_state()
            for k, (x, y) in enumerate(zip(after[0], want)):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (f, k)
            assert after[1] == [1] * len(ps)
        else:                                                               # an open window, or one without a live frame: nothing moved
            assert int(acc.hold.item()) == 1
            for x, y in zip(after[0], before[0]):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f
            assert after[1] == before[1]
            if clip:
                assert opt.grad_stats()["skip"] == 1
    assert acc.stats() == dict(window=2, phase=0, live=0, hold=0, windows=3, frames=6, dropped=3)
    from faster_rcnn_pytorch_amd import parallel
    with pytest.raises(ValueError, match="accumulator.hold"):
        parallel.GraphStep(torch.nn.Linear(2, 2).to(dev), optim.DeviceSGD(ps, lr=lr, guard=skip), lambda f: None, 1, dev, accumulate=2)


# ------------------------------------------------------------------------------------------------ 4. model level
CAP = 6
COUNTS = (2, 5, 0, 1)


def synth(seed, H, W, n, lo, hi):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 3, H, W, generator=g)
    c = torch.rand(n, 2, generator=g) * 0.7 + 0.15
    wh = torch.rand(n, 2, generator=g) * 0.52 + 0.08
    boxes = torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, 1)
    labels = torch.randint(lo, hi, (n,), generator=g)
    return x, boxes, labels


def _frames(seed, counts, H, W, lo, hi, device):
    """Every frame as the device input stage hands it over: CAP rows, a count, NaN in the padding rows."""
    frames = []
    for i, n in enumerate(counts):
        x, b, l = synth(seed + i, H, W, CAP, lo, hi)
        b[n:] = float("nan")
        l[n:] = 1 << 40
        frames.append((x.to(device), b.to(device), l.to(device), torch.tensor([n], dtype=torch.int32, device=device)))
    return frames


def _model(mirror, device, seed=10):
    if mirror == "vgg":
        from faster_rcnn_pytorch_amd.model import FRCNN
        nc = 21
    else:
        from faster_rcnn_pytorch_amd.new_model import FRCNN
        nc = 91
    torch.manual_seed(0)                                                       # identical initial weights everywhere
    model = FRCNN(num_classes=nc, sampling="device", seed=seed).to(device)
    return model, [p for p in model.parameters() if p.requires_grad]


def _sgd(params, guard):
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    return DeviceSGD(params, lr=1e-3, momentum=0.9, weight_decay=1e-4, guard=guard)


def _state(opt, params):
    return [p.detach().clone() for p in params] + [opt.state[p]["momentum_buffer"].detach().clone() for p in params]


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _captured(mirror, device, slot, first, seed=10):
    """Model, optimizer and a captured GraphStep(accumulate=2) over the slot, back at the initial weights and sampling stream."""
    from faster_rcnn_pytorch_amd import parallel
    from faster_rcnn_pytorch_amd.loss import FRCNNLoss
    crit = FRCNNLoss(None)
    model, params = _model(mirror, device, seed)
    init, buffers = [p.detach().clone() for p in params], [b.detach().clone() for b in model.buffers()]

    def forward_loss(f):
        pred, target = model(slot.x, [slot.boxes], [slot.labels], n_gt=slot.n_gt, empty=slot.empty)
        return crit(pred, target), pred
    gs = parallel.GraphStep(model, None, forward_loss, 1, device, accumulate=2, frame_skip=slot.empty, **model.graph_stages())
    opt = _sgd(params, gs.accumulator.hold)
    gs.set_optimizer(opt)
    fresh = copy.deepcopy(opt.state_dict())
    slot.load(*first)
    gs.capture()
    with torch.no_grad():                                                      # in place: what the warm-up window changed goes back
        for p, s in zip(params, init):
            p.copy_(s)
        for b, s in zip(model.buffers(), buffers):
            b.copy_(s)
    opt.load_state_dict(fresh)
    model.sampler.reseed(seed, 1)
    return model, params, opt, gs, init


@pytest.mark.parametrize("mirror", ["vgg", "fpn"])
def test_one_graph_set_accumulates_two_frames_per_update(mirror, monkeypatch):
    from faster_rcnn_pytorch_amd import parallel
    from faster_rcnn_pytorch_amd.loss import FRCNNLoss
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)           # the vendor convolutions of the ResNet body, run to run
    device = torch.device(DEV)
    H, W = (320, 480) if mirror == "vgg" else (320, 448)
    lo, hi = (0, 20) if mirror == "vgg" else (1, 91)
    crit = FRCNNLoss(None)
    frames = _frames(70, COUNTS, H, W, lo, hi, device)

    # ---- the captured step
    slot = parallel.FrameSlot((H, W), CAP, device)
    model, params, opt, gs, init = _captured(mirror, device, slot, frames[0])
    rep = gs.report()
    assert rep["graphs"] == 3 and rep["accumulate"] == 2 and float(gs.seed) == 0.5
    graph_states, holds = [_state(opt, params)], []
    for i, fr in enumerate(frames):
        slot.load(*fr)
        gs.step(i)
        graph_states.append(_state(opt, params))
        holds.append(gs.accumulator.hold.clone())
    torch.cuda.synchronize()
    assert [int(h) for h in holds] == [1, 0, 1, 0]
    st = gs.accumulator.stats()
    assert (st["windows"], st["frames"], st["dropped"]) == (2, 4, 1)
    stream_end = model.sampler.state(device).cpu().tolist()

    # ---- eager accumulation into .grad, on the sliced inputs
    emodel, eparams = _model(mirror, device)
    eopt = _sgd(eparams, torch.zeros(1, dtype=torch.int32, device=device))
    assert _same(init, [p.detach() for p in eparams])
    eager_states = []
    half = torch.tensor(0.5, device=device)
    for k, (x, b, l, cnt) in enumerate(frames):
        n = int(cnt.item())
        if n == 0:
            with torch.no_grad():
                emodel(x, [b], [l], n_gt=cnt)
        else:
            pred, target = emodel(x, [b[:n].contiguous()], [l[:n].contiguous()])
            crit(pred, target)[0].backward(gradient=half)
        if k % 2 == 1:
            eopt.step()
            eopt.zero_grad(set_to_none=True)
        eager_states.append(_state(eopt, eparams))
    torch.cuda.synchronize()
    assert emodel.sampler.state(device).cpu().tolist() == stream_end

    assert _same(graph_states[1], graph_states[0]) and _same(graph_states[3], graph_states[2])      # unchanged after frames 0 and 2
    assert _same(graph_states[2], eager_states[1]), "after the first window"
    assert _same(graph_states[4], eager_states[3]), "after the second window (one frame left out)"
    assert not _same(graph_states[2], graph_states[0]) and not _same(graph_states[4], graph_states[2])
    assert all(bool(torch.isfinite(t).all()) for t in graph_states[4])

    # ---- a window of two frames without boxes changes nothing
    for i in (4, 5):
        slot.load(*frames[2])
        gs.step(i)
        assert int(gs.accumulator.hold.item()) == 1
        assert _same(_state(opt, params), graph_states[4])
    st = gs.accumulator.stats()
    assert (st["windows"], st["frames"], st["dropped"], st["phase"]) == (3, 6, 3, 0)


# ------------------------------------------------------------------------------------------------ 5. two ranks on one GPU over gloo
RANK_COUNTS = ((3, 2, 1, 4), (2, 3, 0, 0))                                  # rank 1's second window is entirely empty
H5, W5 = 320, 480


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from faster_rcnn_pytorch_amd import parallel
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    device = torch.device("cuda", 0)
    frames = _frames(200 + 100 * rank, RANK_COUNTS[rank], H5, W5, 0, 20, device)
    slot = parallel.FrameSlot((H5, W5), CAP, device)
    model, params, opt, gs, _ = _captured("vgg", device, slot, frames[0], seed=10 + rank)
    assert float(gs.seed) == 0.25 and gs.report()["graphs"] == 3
    holds = []
    for i, fr in enumerate(frames):
        slot.load(*fr)
        gs.step(i)
        holds.append(int(gs.accumulator.hold.item()))
    torch.cuda.synchronize()
    q.put((rank, [t.cpu().numpy() for t in _state(opt, params)], holds, gs.accumulator.stats()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_accumulate_and_agree_on_the_step():
    import torch.multiprocessing as mp
    from faster_rcnn_pytorch_amd.loss import FRCNNLoss
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + (os.getpid() + 7) % 1000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    # ---- meanwhile, in this process: each rank's window sum with seed 1/4, the two added, one step
    device = torch.device(DEV)
    crit = FRCNNLoss(None)
    models = [_model("vgg", device, seed=10 + r) for r in range(2)]
    opt = _sgd(models[0][1], torch.zeros(1, dtype=torch.int32, device=device))
    frames = [_frames(200 + 100 * r, RANK_COUNTS[r], H5, W5, 0, 20, device) for r in range(2)]
    quarter = torch.tensor(0.25, device=device)
    for w in range(2):
        for r, (m, ps) in enumerate(models):
            for x, b, l, cnt in frames[r][2 * w:2 * w + 2]:
                n = int(cnt.item())
                if n == 0:
                    with torch.no_grad():
                        m(x, [b], [l], n_gt=cnt)
                else:
                    pred, target = m(x, [b[:n].contiguous()], [l[:n].contiguous()])
                    crit(pred, target)[0].backward(gradient=quarter)
        with torch.no_grad():
            for p0, p1 in zip(models[0][1], models[1][1]):
                p0.grad = p0.grad + (p1.grad if p1.grad is not None else torch.zeros_like(p0))   # an empty window contributes the zeros it wrote
                p1.grad = None
        opt.step()
        opt.zero_grad(set_to_none=True)
        with torch.no_grad():
            for p0, p1 in zip(models[0][1], models[1][1]):
                p1.copy_(p0)
    torch.cuda.synchronize()
    want = [t.cpu().numpy() for t in _state(opt, models[0][1])]

    res = sorted([q.get(timeout=600) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    (_, s0, h0, st0), (_, s1, h1, st1) = res
    for x, y in zip(s0, s1):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))             # identical replicas
    assert h0 == [1, 0, 1, 0] and h1 == [1, 0, 1, 0]                           # MIN over the ranks: rank 1 steps on its empty window too
    assert (st0["dropped"], st1["dropped"], st0["windows"], st1["windows"]) == (0, 2, 2, 2)

    for k, (x, y) in enumerate(zip(s0, want)):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), k
