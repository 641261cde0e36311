"""One captured training step fed from a parallel.FrameSlot: frames with different numbers of ground-truth boxes -- one of them with none --
stream through ONE graph set (GraphStep, n_frames = 1) with DeviceSGD(guard=slot.empty).

Yardstick: eager DeviceSGD steps of the same model on the SLICED inputs (boxes[:n], labels[:n], the classic target-maker entry points),
from the same initial weights and the same position of the device-side sampling stream.  Parameters and momentum are compared bit for
bit after every step, as tests/test_gpu_graph_ddp.py requires of graph versus eager.

The eager reference for the frame WITHOUT boxes is "skip the step": the reference raises on such a frame (docs/PARITY.md), so nothing is
updated.  Its forward is still run on the padded inputs, with n_gt = 0 on the device, because the captured step runs it too and both
target makers draw their value from the sampling stream; its NaN loss is not propagated."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
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


def _state(model, opt, params):
    return [p.detach().clone() for p in params] + [opt.state[p]["momentum_buffer"].detach().clone() for p in params]


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _build(mirror, device, guard):
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    if mirror == "vgg":
        from faster_rcnn_pytorch_amd.model import FRCNN
        nc = 21
    else:
        from faster_rcnn_pytorch_amd.new_model import FRCNN
        nc = 91
    torch.manual_seed(0)                                                       # identical initial weights in both runs
    model = FRCNN(num_classes=nc, sampling="device", seed=10).to(device)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = DeviceSGD(params, lr=1e-3, momentum=0.9, weight_decay=1e-4, guard=guard)
    return model, params, opt


def _restore(model, opt, params, init, buffers, fresh):
    """In place (the graphs hold the addresses): what the capture's warm-up step changed goes back to the initial state."""
    with torch.no_grad():
        for p, s in zip(params, init):
            p.copy_(s)
        for b, s in zip(model.buffers(), buffers):
            b.copy_(s)
    opt.load_state_dict(fresh)
    model.sampler.reseed(10, 1)


@pytest.mark.parametrize("mirror", ["vgg", "fpn"])
def test_frames_with_any_count_stream_through_one_graph_set(mirror, monkeypatch):
    from faster_rcnn_pytorch_amd import parallel
    from faster_rcnn_pytorch_amd.loss import FRCNNLoss
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)           # the vendor convolutions of the ResNet body, run to run
    device = torch.device(DEV)
    H, W = (320, 480) if mirror == "vgg" else (320, 448)
    lo, hi = (0, 20) if mirror == "vgg" else (1, 91)
    crit = FRCNNLoss(None)
    # every frame arrives as the device input stage hands it over: CAP rows, a count, NaN in the padding rows
    frames = []
    for i, n in enumerate(COUNTS):
        x, b, l = synth(70 + i, H, W, CAP, lo, hi)
        b[n:] = float("nan")
        l[n:] = 1 << 40
        frames.append((x.to(device), b.to(device), l.to(device), torch.tensor([n], dtype=torch.int32, device=device)))

    # ---- the captured step
    slot = parallel.FrameSlot((H, W), CAP, device)
    model, params, opt = _build(mirror, device, slot.empty)
    init, buffers = [p.detach().clone() for p in params], [b.detach().clone() for b in model.buffers()]

    def forward_loss(f):
        pred, target = model(slot.x, [slot.boxes], [slot.labels], n_gt=slot.n_gt, empty=slot.empty)
        return crit(pred, target), pred
    fresh = copy.deepcopy(opt.state_dict())
    slot.load(*frames[0])
    gs = parallel.GraphStep(model, opt, forward_loss, 1, device, **model.graph_stages())
    gs.capture()
    assert gs.report()["graphs"] == 3                                          # A, B, U: one set, whatever the frames hold
    _restore(model, opt, params, init, buffers, fresh)
    graph_states, empties = [], []
    for i, fr in enumerate(frames):
        slot.load(*fr)
        gs.step(i)
        graph_states.append(_state(model, opt, params))
        empties.append(slot.empty.clone())
    torch.cuda.synchronize()
    assert [int(e) for e in empties] == [0, 0, 1, 0]
    stream_end = model.sampler.state(device).cpu().tolist()

    # ---- eager steps on the sliced inputs
    guard = torch.zeros(1, dtype=torch.int32, device=device)
    emodel, eparams, eopt = _build(mirror, device, guard)
    assert _same(init, [p.detach() for p in eparams])
    eager_states = []
    for x, b, l, cnt in frames:
        n = int(cnt.item())
        if n == 0:                                                             # "skip the step" (module docstring)
            with torch.no_grad():
                emodel(x, [b], [l], n_gt=cnt)
        else:
            pred, target = emodel(x, [b[:n].contiguous()], [l[:n].contiguous()])
            loss = crit(pred, target)[0]
            eopt.zero_grad(set_to_none=True)
            loss.backward()
            eopt.step()
        eager_states.append(_state(emodel, eopt, eparams))
    torch.cuda.synchronize()
    assert emodel.sampler.state(device).cpu().tolist() == stream_end

    for k, (gst, est) in enumerate(zip(graph_states, eager_states)):
        assert _same(gst, est), "after frame %d (n_gt = %d)" % (k, COUNTS[k])
    assert _same(graph_states[2], graph_states[1])                             # the frame without boxes changed nothing ...
    assert not _same(graph_states[3], graph_states[2])                         # ... and the frame after it trained
    assert all(bool(torch.isfinite(t).all()) for t in graph_states[3])
    from faster_rcnn_pytorch_amd import _lib
    word = int(model.sampler.status.word(device).item())
    assert word & _lib.HT_ERR_GT_COUNT and word & _lib.HT_ERR_SHORT            # reported, without a sync on the way
    assert np.isfinite(stream_end).all()
