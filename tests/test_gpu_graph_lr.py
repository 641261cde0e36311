"""A captured training step that follows the learning-rate schedule (optim.DeviceSGD inside parallel.GraphStep).

The reference steps MultiStepLR once per epoch (main.py:58-65).  A torch optimizer with a Python-float lr is frozen at capture; DeviceSGD
reads lr / momentum / weight decay from device memory at replay; opt.push_hyper() carries a scheduler's change there, outside the graphs.  A three-layer MLP with two resident frames is trained as graph replays;
after every replay the gradients the replay produced are copied to the host and a torch.optim.SGD + MultiStepLR twin on the CPU is
advanced with them: parameters equal bit for bit at every step, through milestones, a mid-run load_state_dict and a guarded step."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=5e-2, momentum=0.9, weight_decay=5e-4)


def _mlp():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(13, 32), torch.nn.ReLU(), torch.nn.Linear(32, 17), torch.nn.ReLU(), torch.nn.Linear(17, 5))


def _frames():
    g = torch.Generator().manual_seed(1)
    return [(torch.randn(8, 13, generator=g).to(DEV), torch.randn(8, 5, generator=g).to(DEV)) for _ in range(2)]


class _Run(object):
    """One replica on the GPU under GraphStep (graphs or eager pieces) with DeviceSGD + MultiStepLR([1, 2])."""

    def __init__(self, graphs, guard=None):
        from faster_rcnn_pytorch_amd import parallel
        from faster_rcnn_pytorch_amd.optim import DeviceSGD
        self.model = _mlp().to(DEV)
        self.frames = _frames()
        self.opt = DeviceSGD(self.model.parameters(), guard=guard, **HYPER)
        self.sched = torch.optim.lr_scheduler.MultiStepLR(self.opt, milestones=[1, 2], gamma=0.1)

        def forward_loss(f):
            x, y = self.frames[f]
            out = self.model(x)
            return [torch.nn.functional.mse_loss(out, y)], (out, out)
        self.gs = parallel.GraphStep(self.model, self.opt, forward_loss, 2, torch.device(DEV), graphs=graphs)
        init = [p.detach().clone() for p in self.model.parameters()]
        fresh = copy.deepcopy(self.opt.state_dict())                      # nothing born yet
        self.gs.capture()                                                  # its warm-up passes step the weights and bear the momenta:
        with torch.no_grad():                                              # back to the initial state, in place
            for p, s in zip(self.model.parameters(), init):
                p.copy_(s)
        self.opt.load_state_dict(fresh)
        assert self.opt.born() == [0] * 6
        assert (self.gs.gU is not None) == graphs

    def params(self):
        torch.cuda.synchronize()
        return [p.detach().cpu().numpy().copy() for p in self.model.parameters()]

    def grads(self):
        torch.cuda.synchronize()
        return [self.gs.views[id(p)].detach().cpu().clone() for p in self.model.parameters()]


class _Twin(object):
    """torch.optim.SGD + MultiStepLR on the CPU, fed with the gradients a replay produced."""

    def __init__(self):
        self.model = _mlp()
        self.opt = torch.optim.SGD(self.model.parameters(), **HYPER)
        self.sched = torch.optim.lr_scheduler.MultiStepLR(self.opt, milestones=[1, 2], gamma=0.1)

    def step(self, grads):
        for p, g in zip(self.model.parameters(), grads):
            p.grad = g
        self.opt.step()

    def params(self):
        return [p.detach().numpy().copy() for p in self.model.parameters()]


def _equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_replayed_step_follows_multisteplr_and_equals_torch_sgd_on_the_cpu_and_the_eager_path():
    run, eager, twin = _Run(True), _Run(False), _Twin()
    assert run.gs.report()["graphs"] == 2 + 1
    addr = [run.opt.state[p]["momentum_buffer"].data_ptr() for p in run.model.parameters()]
    lrs, i = [], 0
    for epoch in range(3):
        for _ in range(2):
            run.gs.step(i), eager.gs.step(i)
            twin.step(run.grads())
            assert _equal(run.params(), twin.params()), ("graph replay vs torch.optim.SGD on the CPU", epoch, i)
            assert _equal(run.params(), eager.params()), ("graph replay vs eager DeviceSGD", epoch, i)
            lrs.append(run.opt.param_groups[0]["lr"])
            i += 1
        run.sched.step(), eager.sched.step(), twin.sched.step()
        run.opt.push_hyper()                                               # the new lr to the device block: outside the graphs, no sync
    assert lrs[0] == lrs[1] == 5e-2 and lrs[2] == lrs[3] == pytest.approx(5e-3) and lrs[4] == lrs[5] == pytest.approx(5e-4)
    assert [g["lr"] for g in run.opt.param_groups] == [g["lr"] for g in twin.opt.param_groups]
    assert run.opt.born() == [1] * 6 and addr == [run.opt.state[p]["momentum_buffer"].data_ptr() for p in run.model.parameters()]
    # the schedule is visible in the weights: a twin whose lr stays at the captured value ends somewhere else
    frozen, again = _Twin(), _Run(True)
    for j in range(4):
        again.gs.step(j)
        frozen.step(again.grads())
        if j == 1:
            again.sched.step()                                             # only the replayed run's lr drops
            again.opt.push_hyper()
    assert not _equal(again.params(), frozen.params())


def test_load_state_dict_into_a_captured_optimizer_continues_the_trajectory():
    run, twin = _Run(True), _Twin()
    addr = [run.opt.state[p]["momentum_buffer"].data_ptr() for p in run.model.parameters()]
    saved = None
    for i in range(4):
        run.gs.step(i)
        twin.step(run.grads())
        if i % 2 == 1:
            run.sched.step(), twin.sched.step()
            run.opt.push_hyper()
        if i == 1:                                                         # a checkpoint after the first epoch
            saved = (copy.deepcopy(twin.model.state_dict()), copy.deepcopy(twin.opt.state_dict()), copy.deepcopy(twin.sched.state_dict()))
    assert _equal(run.params(), twin.params())
    after4 = run.params()
    # resume both from the checkpoint: weights in place, torch's optimizer state INTO the captured optimizer
    twin.model.load_state_dict(saved[0]), twin.opt.load_state_dict(saved[1]), twin.sched.load_state_dict(saved[2])
    with torch.no_grad():
        for p, (_, v) in zip(run.model.parameters(), saved[0].items()):
            p.copy_(v)
    run.opt.load_state_dict(saved[1]), run.sched.load_state_dict(saved[2])
    assert addr == [run.opt.state[p]["momentum_buffer"].data_ptr() for p in run.model.parameters()]
    assert run.opt.param_groups[0]["lr"] == twin.opt.param_groups[0]["lr"] == pytest.approx(5e-3)
    for i in range(2, 4):
        run.gs.step(i)
        twin.step(run.grads())
        assert _equal(run.params(), twin.params()), i
    assert _equal(run.params(), after4)                                    # the same two steps as before the resume


def test_guarded_replay_changes_nothing_and_the_next_one_catches_up():
    guard = torch.zeros(1, dtype=torch.int32, device=DEV)
    run, twin = _Run(True, guard=guard), _Twin()
    run.gs.step(0)
    twin.step(run.grads())
    assert _equal(run.params(), twin.params())
    guard.fill_(1)
    run.gs.step(1)                                                         # forward and backward run, the update does not
    moms = [run.opt.state[p]["momentum_buffer"].cpu().numpy() for p in run.model.parameters()]
    assert _equal(run.params(), twin.params())                             # the twin did not step either
    assert _equal(moms, [twin.opt.state[p]["momentum_buffer"].numpy() for p in twin.model.parameters()])
    guard.fill_(0)
    run.gs.step(2)
    twin.step(run.grads())
    assert _equal(run.params(), twin.params())
    # and a guard raised before the very first update leaves every tensor unborn
    guard.fill_(1)
    first = _Run(True, guard=guard)
    first.gs.step(0)
    torch.cuda.synchronize()
    assert first.opt.born() == [0] * 6 and first.opt.state_dict()["state"] == {}
    guard.fill_(0)
    first.gs.step(0)
    t2 = _Twin()
    t2.step(first.grads())
    assert _equal(first.params(), t2.params())


def test_vgg_mirror_step_captured_with_device_sgd_equals_the_eager_device_sgd_step():
    """The wiring, once, on the real model at the frame size of tests/test_gpu_graph.py: the weights the replayed optimizer graph leaves
    equal those of an eager DeviceSGD step taken from the same weights with the gradients that replay produced."""
    from faster_rcnn_pytorch_amd import parallel
    from faster_rcnn_pytorch_amd.loss import FRCNNLoss
    from faster_rcnn_pytorch_amd.model import FRCNN
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    H, W = 600, 1000
    device = torch.device(DEV)
    torch.manual_seed(0)
    model = FRCNN(num_classes=21, sampling="device", seed=10).to(device)
    crit = FRCNNLoss(None)
    g = torch.Generator().manual_seed(50)
    x = torch.randn(1, 3, H, W, generator=g).to(device)
    c = torch.rand(3, 2, generator=g) * 0.7 + 0.15
    wh = torch.rand(3, 2, generator=g) * 0.52 + 0.08
    boxes = torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, 1).to(device)
    labels = torch.randint(0, 20, (3,), generator=g).to(device)
    params = [p for p in model.parameters() if p.requires_grad]
    hyper = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)
    opt = DeviceSGD(params, **hyper)

    def forward_loss(f):
        pred, target = model(x, [boxes], [labels])
        return crit(pred, target), pred
    gs = parallel.GraphStep(model, opt, forward_loss, 1, device, **model.graph_stages())
    init = [p.detach().clone() for p in params]
    fresh = copy.deepcopy(opt.state_dict())
    gs.capture()
    with torch.no_grad():
        for p, s in zip(params, init):
            p.copy_(s)
    opt.load_state_dict(fresh)
    opt.param_groups[0]["lr"] = 5e-4                                       # changed after the capture: the replay must use it
    opt.push_hyper()
    gs.step(0)
    torch.cuda.synchronize()
    model.check_device_status()
    twins = [torch.nn.Parameter(s) for s in init]                         # the initial weights, now owned by the eager optimizer
    for t, p in zip(twins, params):
        t.grad = gs.views[id(p)].clone()
    eager = DeviceSGD(twins, **dict(hyper, lr=5e-4))
    eager.step()
    torch.cuda.synchronize()
    assert opt.born() == eager.born() == [1] * len(params)
    for t, p in zip(twins, params):
        assert torch.equal(t.detach().view(torch.int32), p.detach().view(torch.int32))
        assert torch.equal(eager.state[t]["momentum_buffer"].view(torch.int32), opt.state[p]["momentum_buffer"].view(torch.int32))
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert all(float(opt.state[p]["momentum_buffer"].abs().sum()) > 0 for p in params)       # a step did happen


def test_whole_step_capture_of_integration_md_follows_the_schedule():
    """The single-GPU pattern of INTEGRATION.md: zero_grad(set_to_none=False), forward, backward and opt.launch() in ONE graph;
    push_hyper() in front of every replay.  Two epochs of two steps against the CPU twin."""
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    model, twin = _mlp().to(DEV), _Twin()
    x, y = _frames()[0]
    opt = DeviceSGD(model.parameters(), **HYPER)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1, 2], gamma=0.1)
    init = [p.detach().clone() for p in model.parameters()]
    fresh = copy.deepcopy(opt.state_dict())

    def body(update):
        opt.zero_grad(set_to_none=False)
        torch.nn.functional.mse_loss(model(x), y).backward()
        update()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body(opt.step)                                                     # creates the gradient tensors and the table
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    opt.push_hyper(), opt.prepare()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body(opt.launch)
    with torch.no_grad():
        for p, s in zip(model.parameters(), init):
            p.copy_(s)
    opt.load_state_dict(fresh)
    for epoch in range(2):
        for _ in range(2):
            opt.push_hyper()
            g.replay()
            torch.cuda.synchronize()
            twin.step([p.grad.detach().cpu().clone() for p in model.parameters()])
            assert _equal([p.detach().cpu().numpy() for p in model.parameters()], twin.params()), epoch
        sched.step(), twin.sched.step()
    assert opt.param_groups[0]["lr"] == twin.opt.param_groups[0]["lr"] == pytest.approx(5e-4)
