"""A captured training step that clips its gradients and survives a diverged frame (optim.DeviceSGD(max_grad_norm=, skip_nonfinite=True)
inside parallel.GraphStep; the small MLP of tests/test_gpu_graph_lr.py).

Three resident frames are trained as graph replays; the second frame carries a NaN input, so its forward, loss and every gradient are
NaN.  That replay changes nothing -- parameters, momenta, born words -- and is counted; every other replay equals a torch.optim.SGD twin
on the CPU that never sees the bad frame and is fed g.mul_(coef) with the coefficient read back from the device, and equals the eager
DeviceSGD path, bit for bit.  max_grad_norm is changed twice between replays: push_hyper() carries it, nothing is recaptured."""
import copy
import gc

import numpy as np
import pytest
import torch

import grad_norm_ref as gn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=5e-2, momentum=0.9, weight_decay=5e-4)
BAD_FRAME = 1
MAX_NORM = (0.1, 0.2, 10.0)                          # per cycle of three frames; the gradient norms of this MLP are 0.3 .. 0.6


def _mlp():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(13, 32), torch.nn.ReLU(), torch.nn.Linear(32, 17), torch.nn.ReLU(), torch.nn.Linear(17, 5))


def _frames():
    g = torch.Generator().manual_seed(1)
    frames = [(torch.randn(8, 13, generator=g), torch.randn(8, 5, generator=g)) for _ in range(3)]
    frames[BAD_FRAME][0][3, 7] = float("nan")
    return [(x.to(DEV), y.to(DEV)) for x, y in frames]


class _Run(object):
    """One replica on the GPU under GraphStep (graphs or eager pieces) with a clipping, skipping DeviceSGD."""

    def __init__(self, graphs):
        from faster_rcnn_pytorch_amd import parallel
        from faster_rcnn_pytorch_amd.optim import DeviceSGD
        self.model = _mlp().to(DEV)
        self.frames = _frames()
        self.opt = DeviceSGD(self.model.parameters(), max_grad_norm=MAX_NORM[0], skip_nonfinite=True, **HYPER)

        def forward_loss(f):
            x, y = self.frames[f]
            out = self.model(x)
            return [torch.nn.functional.mse_loss(out, y)], (out, out)
        self.gs = parallel.GraphStep(self.model, self.opt, forward_loss, 3, torch.device(DEV), graphs=graphs)
        init = [p.detach().clone() for p in self.model.parameters()]
        fresh = copy.deepcopy(self.opt.state_dict())                      # nothing born yet
        self.gs.capture()                                                  # its warm-up passes step the weights (and skip the bad frame once)
        with torch.no_grad():
            for p, s in zip(self.model.parameters(), init):
                p.copy_(s)
        self.opt.load_state_dict(fresh)
        assert self.opt.born() == [0] * 6 and (self.gs.gU is not None) == graphs
        if graphs:                                                         # the counters are not checkpointed: the warm-up's stay
            st = self.opt.grad_stats()
            assert (st["steps"], st["skipped_steps"]) == (3, 1)
            self.base = (3, 1)
        else:
            self.base = (0, 0)

    def state(self):
        torch.cuda.synchronize()
        ps = [p.detach().cpu().numpy().copy() for p in self.model.parameters()]
        ms = [self.opt.state[p]["momentum_buffer"].cpu().numpy().copy() for p in self.model.parameters()]
        return ps, ms, self.opt.born()

    def grads(self):
        torch.cuda.synchronize()
        return [self.gs.views[id(p)].detach().cpu().clone() for p in self.model.parameters()]


class _Twin(object):
    """torch.optim.SGD on the CPU, fed with the gradients a replay produced, scaled in place as clip_grad_norm_ does."""

    def __init__(self):
        self.model = _mlp()
        self.opt = torch.optim.SGD(self.model.parameters(), **HYPER)

    def step(self, grads, coef):
        for p, g in zip(self.model.parameters(), grads):
            p.grad = g.clone()
            p.grad.mul_(coef)
        self.opt.step()

    def params(self):
        return [p.detach().numpy().copy() for p in self.model.parameters()]


def _equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_replayed_clipped_step_skips_the_nan_frame_and_equals_torch_on_the_cpu_and_the_eager_path():
    run, eager, twin = _Run(True), _Run(False), _Twin()
    assert run.gs.report()["graphs"] == 3 + 1
    block = (run.opt._gn_state.data_ptr(), run.opt._gn_work.data_ptr())
    coefs, skipped = [], 0
    for i in range(9):
        if i % 3 == 0:
            run.opt.max_grad_norm = eager.opt.max_grad_norm = MAX_NORM[i // 3]
            run.opt.push_hyper()                                           # to the device block: outside the graphs, no sync, no recapture
        before = run.state()
        run.gs.step(i), eager.gs.step(i)
        st, st_e = run.opt.grad_stats(), eager.opt.grad_stats()
        assert st["steps"] - run.base[0] == st_e["steps"] == i + 1
        if i % 3 == BAD_FRAME:
            skipped += 1
            assert st["skip"] == st_e["skip"] == 1 and st["nonfinite"] == st_e["nonfinite"] == sum(p.numel() for p in run.model.parameters())
            assert np.isnan(st["norm"]) and np.isnan(st["coef"]) and bool(torch.isnan(run.opt.grad_norm_tensor))
            after = run.state()
            assert _equal(before[0], after[0]) and _equal(before[1], after[1]) and before[2] == after[2], "a skipped replay wrote something"
        else:
            grads = run.grads()
            want = gn.state_after([g.numpy() for g in grads], MAX_NORM[i // 3], gn.CLIP | gn.SKIP_NONFINITE)
            assert st["skip"] == 0 and st["nonfinite"] == 0 and gn.f64_bits(st["sumsq"]) == gn.f64_bits(want["sumsq"])
            assert gn.f32_bits(st["coef"]) == gn.f32_bits(want["coef"]) == gn.f32_bits(st_e["coef"])      # the max_grad_norm of THIS cycle
            twin.step(grads, st["coef"])
            coefs.append(st["coef"])
        assert st["skipped_steps"] - run.base[1] == st_e["skipped_steps"] == skipped
        assert _equal(run.state()[0], twin.params()), ("graph replay vs torch.optim.SGD on the CPU", i)
        assert _equal(run.state()[0], eager.state()[0]) and _equal(run.state()[1], eager.state()[1]), ("graph replay vs eager DeviceSGD", i)
    assert all(0 < c < 1 for c in coefs[:4]) and all(a < b for a, b in zip(coefs[:2], coefs[2:4])) and coefs[4:] == [1.0, 1.0]
    assert skipped == 3 and run.opt.born() == [1] * 6 and block == (run.opt._gn_state.data_ptr(), run.opt._gn_work.data_ptr())
    assert all(np.isfinite(p).all() for p in run.state()[0])
    del run, eager                                                         # a _Run is a cycle (forward_loss refers back to it) that holds graphs:
    gc.collect()                                                           # destroyed here, not by a collection inside a later test's capture
