"""The training telemetry under HIP graphs (telemetry.TensorStats / ScalarJournal, DeviceSGD(tensor_stats=, after_step=),
parallel.GraphStep(record=)): replays leave the bits the eager calls leave -- rows, state, rings, marks, totals -- and with both
DeviceSGD arguments None nothing is launched or allocated that was not before.  The MLP and frames are tests/test_gpu_graph_lr.py's."""
import copy
import gc

import pytest
import torch

import test_gpu_graph_lr as glr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5), (9000,), (1,), (257,)]


def _toy(every):
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    from faster_rcnn_pytorch_amd.telemetry import ScalarJournal, TensorStats
    gen = torch.Generator().manual_seed(51)
    params = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).to(DEV)) for s in SHAPES]
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = DeviceSGD(params, lr=1e-2, momentum=0.9, max_grad_norm=0.5)
    opt.push_hyper(), opt.prepare()
    return opt, params, TensorStats(opt, every=every), ScalarJournal(["grad_norm", "twice", "lr"], 4, DEV)


def _grads(k):
    gen = torch.Generator().manual_seed(100 + k)
    return [torch.randn(*s, generator=gen) * 0.05 for s in SHAPES]


def _measure_and_append(opt, stats, journal):
    """measure() plus append; `twice` is a journal source allocated right here -- inside the capture's pool when captured."""
    stats.measure()
    views = opt.scalar_views()
    twice = (views["grad_norm"] * 2).to(torch.float64)
    journal.append([views["grad_norm"], twice, views["lr/0"]])


def _run_toy(graph, every=2):
    opt, params, stats, journal = _toy(every)
    g = None
    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _measure_and_append(opt, stats, journal)                             # warm-up
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        stats.reset(), journal.reset()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _measure_and_append(opt, stats, journal)
    out = []
    for k in range(5):
        for p, v in zip(params, _grads(k)):
            p.grad.copy_(v)
        opt.step()                                                        # eager in both runs: moves the weights and the state block's norm
        if graph:
            g.replay()
        else:
            _measure_and_append(opt, stats, journal)
        torch.cuda.synchronize()
        out.append((stats._block.cpu().clone(), journal._block.cpu().clone()))
    return out, stats, journal


def test_five_replays_of_measure_and_append_equal_five_eager_calls():
    eager, _, _ = _run_toy(False)
    replay, stats, journal = _run_toy(True)
    for k, ((a, b), (c, d)) in enumerate(zip(eager, replay)):
        assert torch.equal(a, c), ("rows | state", k)
        assert torch.equal(b, d), ("journal", k)
    got = stats.read()
    assert (got["tick"], got["measures"], got["measured_tick"]) == (5, 3, 4)           # every = 2: replays 0, 2 and 4 measured, decided on the device
    assert not torch.equal(replay[2][0][64:], replay[1][0][64:]) and torch.equal(replay[3][0][64:], replay[2][0][64:])      # rows move on measuring ticks only
    data = journal.read()
    assert data["cursor"] == 5 and len(data["rows"]) == 4 and (data["rows"][:, 1] == 2 * data["rows"][:, 0]).all() and (data["rows"][:, 0] > 0).all()
    assert len(set(data["rows"][:, 0].tolist())) == 4                     # changing data: every replay saw its own norm
    assert set(data["rows"][:, 2].tolist()) == {float(torch.tensor(1e-2, dtype=torch.float32))}


class _Run(object):
    """GraphStep over the MLP with DeviceSGD(tensor_stats=, after_step=) and record=: two journals, losses per frame, scalars per update."""

    def __init__(self, graphs, accumulate):
        from faster_rcnn_pytorch_amd import parallel
        from faster_rcnn_pytorch_amd.optim import DeviceSGD
        from faster_rcnn_pytorch_amd.telemetry import ScalarJournal
        self.model, self.frames = glr._mlp().to(DEV), glr._frames()
        self.losses = ScalarJournal(["loss", "frame"], 16, DEV)
        self.updates = ScalarJournal(["lr", "grad_norm", "clip_coef", "skip", "nonfinite"], 16, DEV)
        self.frame_word = [torch.full((1,), f, dtype=torch.int32, device=DEV) for f in range(2)]

        def forward_loss(f):
            x, y = self.frames[f]
            out = self.model(x)
            return [torch.nn.functional.mse_loss(out, y)], (out, out)

        def record(f, losses):
            self.losses.append([losses[0].reshape(1), self.frame_word[f]], mark=self.frame_word[f])

        def after_step():
            v = self.opt.scalar_views()
            self.updates.append([v["lr/0"], v["grad_norm"], v["clip_coef"], v["skip"], v["nonfinite"]])
        kw = dict(max_grad_norm=0.2, skip_nonfinite=True, tensor_stats=True, after_step=after_step, **glr.HYPER)
        if accumulate == 1:
            self.opt = DeviceSGD(self.model.parameters(), **kw)
            self.gs = parallel.GraphStep(self.model, self.opt, forward_loss, 2, torch.device(DEV), record=record, graphs=graphs)
        else:
            self.gs = parallel.GraphStep(self.model, None, forward_loss, 2, torch.device(DEV), record=record, graphs=graphs, accumulate=accumulate)
            self.opt = DeviceSGD(self.model.parameters(), guard=self.gs.accumulator.hold, **kw)
            self.gs.set_optimizer(self.opt)
        init = [p.detach().clone() for p in self.model.parameters()]
        fresh = copy.deepcopy(self.opt.state_dict())
        self.gs.capture()                                                  # the warm-up passes step, measure and append: start over
        with torch.no_grad():
            for p, s in zip(self.model.parameters(), init):
                p.copy_(s)
        self.opt.load_state_dict(fresh)
        self.gs.reset_window()
        self.losses.reset(), self.updates.reset(), self.opt.tensor_stats.reset()

    def blocks(self):
        torch.cuda.synchronize()
        return [b.cpu().clone() for b in (self.losses._block, self.updates._block, self.opt.tensor_stats._block)]


@pytest.mark.parametrize("accumulate", [1, 2])
def test_graphstep_replays_leave_the_eager_runs_journals_and_rows(accumulate):
    run, eager = _Run(True, accumulate), _Run(False, accumulate)
    assert run.gs.gU is not None and eager.gs.gU is None
    for i in range(6):
        run.gs.step(i), eager.gs.step(i)
        for name, a, b in zip(("losses", "updates", "rows | state"), run.blocks(), eager.blocks()):
            assert torch.equal(a, b), (name, i)
    losses, updates, stats = run.losses.read(), run.updates.read(), run.opt.tensor_stats.read()
    assert losses["cursor"] == 6 and updates["cursor"] == 6 // accumulate == stats["tick"] == stats["measures"]      # K loss rows per update row
    assert losses["marks"].tolist() == [0, 1] * 3 and losses["rows"][:, 1].tolist() == [0.0, 1.0] * 3 and (losses["rows"][:, 0] > 0).all()
    assert (updates["rows"][:, 0] == float(torch.tensor(glr.HYPER["lr"], dtype=torch.float32))).all() and (updates["rows"][:, 1] > 0).all()
    assert (updates["rows"][:, 3:] == 0).all() and stats["first_nonfinite_g"] is None
    assert all(t["grad_norm"] > 0 and t["weight_norm"] > 0 for t in stats["tensors"].values())
    sm = run.losses.smoothed(window=4)
    assert sm["loss"]["count"] == 6 and sm["loss"]["value"] == losses["rows"][-1, 0] and sm["frame"]["median"] == 0.0
    del run, eager
    gc.collect()


def test_both_arguments_none_is_the_old_path():
    from faster_rcnn_pytorch_amd import _lib
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    p = torch.nn.Parameter(torch.zeros(8, device=DEV))
    p.grad = torch.ones(8, device=DEV)
    plain = DeviceSGD([p], lr=0.1, momentum=0.9)
    assert plain.tensor_stats is None and plain.after_step is None
    _lib.prof_reset(), _lib.prof_enable(True)
    try:
        plain.step()
        torch.cuda.synchronize()
        launched = {k: n for k, (_, n) in _lib.prof_report().items()}
        assert launched == {"sgd_update_kernel": 1, "sgd_born_kernel": 1}, launched
        _lib.prof_reset()
        seen = []
        both = DeviceSGD([p], lr=0.1, momentum=0.9, skip_nonfinite=True, tensor_stats=True, after_step=lambda: seen.append(1))
        both.step()
        torch.cuda.synchronize()
        launched = {k: n for k, (_, n) in _lib.prof_report().items()}
        assert launched == {"tensor_stats_partial_kernel": 1, "tensor_stats_finish_kernel": 1, "tensor_stats_advance_kernel": 1, "grad_norm_partial_kernel": 1,
                            "grad_norm_finish_kernel": 1, "sgd_update_kernel": 1, "sgd_born_kernel": 1}, launched
        assert seen == [1]
    finally:
        _lib.prof_enable(False), _lib.prof_reset()
    assert plain._gn_state is None and plain._gn_work is None and sorted(plain.scalar_views()) == ["lr/0"]
    for bad in (3, "yes", [1]):
        with pytest.raises(TypeError, match="tensor_stats must be True or a dict"):
            DeviceSGD([p], lr=0.1, tensor_stats=bad)
    with pytest.raises(TypeError, match="after_step must be callable"):
        DeviceSGD([p], lr=0.1, after_step=3)
    with pytest.raises(ValueError, match="names must be 1 strings"):
        DeviceSGD([p], lr=0.1, tensor_stats=dict(names=["a", "b"]))


def test_a_pending_every_is_refused_while_the_stream_is_capturing(monkeypatch):
    """The rule of the lr: the device block is written outside graphs.  (No capture is begun here: the check is the object's own.)"""
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    from faster_rcnn_pytorch_amd.telemetry import ScalarJournal
    p = torch.nn.Parameter(torch.ones(8, device=DEV))
    p.grad = torch.ones(8, device=DEV)
    opt, journal = DeviceSGD([p], lr=0.1, tensor_stats=True), ScalarJournal(["a"], 2, DEV)
    opt.push_hyper(), opt.prepare()
    opt.tensor_stats.every = 4                                            # not pushed
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="every changed and the stream is capturing"):
            opt.launch()
        with pytest.raises(RuntimeError, match="every changed and the stream is capturing"):
            opt.tensor_stats.measure()
        with pytest.raises(RuntimeError, match="reset\\(\\) while the stream is capturing"):
            journal.reset()
    assert opt.tensor_stats.read()["tick"] == 0                           # nothing was launched
    opt.step()
    got = opt.tensor_stats.read()
    assert (got["every"], got["tick"], got["measures"]) == (4, 1, 1)
