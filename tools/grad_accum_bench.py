"""GPU time of the device-side gradient accumulation (csrc/grad_accum.hip) and what it does to the step rate; recorded, never asserted.

    python tools/grad_accum_bench.py [--replays 50] [--rounds 9] [--warmup 10] [--steps 16] [--step-rounds 3] [--out profiles/grad_accum_bench.json]

op      For the trainable-parameter shapes of both mirrors (model.FRCNN: VGG16, new_model.FRCNN: ResNet-50-FPN): the accumulators are views
        into ONE flat fp32 buffer at the offsets parallel.GraphStep gives them (so a view behind an odd-sized tensor is misaligned), the
        sources are separate allocations as autograd's are.  Graphs captured once each, GPU time per replay = HIP-event time around
        `replays` back-to-back replays / replays, alternating inside every round after `warmup` replays of each:
          accumulate_first     optim.GradAccumulator.accumulate at phase 0 (acc = src: 8 B per element)
          accumulate_later     the same call at phase 1 of a window of 2 (acc += src: 12 B per element)
          accumulate_skipped   phase 1, frame_skip != 0 (nothing is read or written)
          foreach_copy         torch._foreach_copy_ on the same tensors (what GraphStep._store does with accumulate=1)
          foreach_add          torch._foreach_add_ on the same tensors
          same_bytes_copy      one device copy of a flat buffer of the gradients' size
        The phase is set outside the graphs and no advance() is captured, so every replay of a graph takes the same branch.
steps   steps per second of a parallel.GraphStep stream over a parallel.FrameSlot with optim.DeviceSGD, in a fresh child process per
        mirror under a time limit (--limit), at accumulate = 1, 2, 4, 8 (alternating inside every round; wall time around `steps` steps
        ending in one synchronisation; `steps` is a multiple of 8 so that every K closes whole windows).

Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tools")) if p not in sys.path]

SIZES = {"vgg16": dict(H=600, W=1000, num_classes=21, lo=0, hi=20), "resnet50_fpn": dict(H=800, W=1344, num_classes=91, lo=1, hi=91)}
KS = (1, 2, 4, 8)
CAP = 8


def _stats(v, per):
    import numpy as np
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "per_round": per, "rounds": len(v)}


# ------------------------------------------------------------------------------------------------ the op alone
def part_op(which, a):
    import torch
    from faster_rcnn_pytorch_amd.optim import GradAccumulator
    from sgd_bench import capture, model_shapes
    dev = torch.device("cuda:0")
    shapes = model_shapes(which)
    gen = torch.Generator().manual_seed(0)
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    flat = torch.zeros(n, device=dev)
    accs, off = [], 0
    for s in shapes:
        k = int(torch.Size(s).numel())
        accs.append(flat[off:off + k].view(s))
        off += k
    srcs = [(torch.randn(*s, generator=gen) * 0.02).to(dev) for s in shapes]
    skip_on = torch.ones(1, dtype=torch.int32, device=dev)
    first, later, skipped = GradAccumulator(2, dev), GradAccumulator(2, dev), GradAccumulator(2, dev, frame_skip=skip_on)
    later.advance()
    skipped.advance()                                                          # both at phase 1 from here on: no advance() is captured
    a_flat, b_flat = torch.randn(n, device=dev), torch.empty(n, device=dev)
    fns = {"accumulate_first": lambda: first.accumulate(accs, srcs), "accumulate_later": lambda: later.accumulate(accs, srcs),
           "accumulate_skipped": lambda: skipped.accumulate(accs, srcs), "foreach_copy": lambda: torch._foreach_copy_(accs, srcs),
           "foreach_add": lambda: torch._foreach_add_(accs, srcs), "same_bytes_copy": lambda: b_flat.copy_(a_flat)}
    graphs = {k: capture(f) for k, f in fns.items()}
    for g in graphs.values():
        for _ in range(a.warmup):
            g.replay()
    torch.cuda.synchronize()
    t = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():                                            # alternating: every round times each graph
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                g.replay()
            e1.record()
            e1.synchronize()
            t[k].append(1e3 * e0.elapsed_time(e1) / a.replays)
    assert (first.stats()["phase"], later.stats()["phase"], skipped.stats()["phase"]) == (0, 1, 1)
    misaligned = sum(1 for x in accs if x.data_ptr() % 16)
    r = {"tensors": len(shapes), "elements": n, "gradient_bytes": 4 * n, "chunks": sum((x.numel() + 8191) // 8192 for x in accs),
         "accumulators_not_16_byte_aligned": misaligned, "elements_on_the_dword_path": sum(x.numel() for x in accs if x.data_ptr() % 16)}
    for k in graphs:
        r[k + "_us"] = _stats(t[k], a.replays)
    med = {k: r[k + "_us"]["median"] for k in graphs}
    r["accumulate_first_tb_per_s"] = 8 * n / (med["accumulate_first"] * 1e-6) / 1e12
    r["accumulate_later_tb_per_s"] = 12 * n / (med["accumulate_later"] * 1e-6) / 1e12
    r["same_bytes_copy_tb_per_s"] = 8 * n / (med["same_bytes_copy"] * 1e-6) / 1e12
    r["accumulate_first_over_foreach_copy"] = med["accumulate_first"] / med["foreach_copy"]
    r["accumulate_later_over_foreach_add"] = med["accumulate_later"] / med["foreach_add"]
    return r


# ------------------------------------------------------------------------------------------------ the step rate
def part_steps(which, a):
    import torch
    from faster_rcnn_pytorch_amd import parallel
    from faster_rcnn_pytorch_amd.loss import FRCNNLoss
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    from train_stream_bench import _boxes
    cfg = SIZES[which]
    if which == "vgg16":
        from faster_rcnn_pytorch_amd.model import FRCNN
    else:
        from faster_rcnn_pytorch_amd.new_model import FRCNN
    device = torch.device("cuda:0")
    crit = FRCNNLoss(None)
    hyper = dict(lr=2e-3, momentum=0.9, weight_decay=5e-4)
    frames = []
    for i in range(8):
        g = torch.Generator().manual_seed(1000 + i)
        k = 1 + (3 * i) % CAP
        b, l = torch.zeros(CAP, 4), torch.zeros(CAP, dtype=torch.int64)
        b[:k] = _boxes(g, k, 0.08, 0.6)
        l[:k] = torch.randint(cfg["lo"], cfg["hi"], (k,), generator=g)
        frames.append((torch.randn(1, 3, cfg["H"], cfg["W"], generator=g).to(device), b.to(device), l.to(device),
                       torch.tensor([k], dtype=torch.int32, device=device)))
    ways, reports, models = {}, {}, []
    for K in KS:
        torch.manual_seed(0)
        model = FRCNN(num_classes=cfg["num_classes"], sampling="device", seed=1).to(device)
        params = [p for p in model.parameters() if p.requires_grad]
        slot = parallel.FrameSlot((cfg["H"], cfg["W"]), CAP, device)

        def forward_loss(f, model=model, slot=slot):
            pred, target = model(slot.x, [slot.boxes], [slot.labels], n_gt=slot.n_gt, empty=slot.empty)
            return crit(pred, target), pred
        slot.load(*frames[0])
        if K == 1:
            gs = parallel.GraphStep(model, DeviceSGD(params, guard=slot.empty, **hyper), forward_loss, 1, device, **model.graph_stages())
        else:
            gs = parallel.GraphStep(model, None, forward_loss, 1, device, accumulate=K, frame_skip=slot.empty, **model.graph_stages())
            gs.set_optimizer(DeviceSGD(params, guard=gs.accumulator.hold, **hyper))
        gs.capture()

        def step(i, gs=gs, slot=slot):
            slot.load(*frames[i % len(frames)])
            gs.step(i)
        ways[K], reports[K] = step, gs.report()
        models.append(model)
    for fn in ways.values():
        for i in range(8):
            fn(i)
    torch.cuda.synchronize()
    t = {K: [] for K in ways}
    for _ in range(a.step_rounds):
        for K, fn in ways.items():                                             # alternating: every round times each K
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                fn(i)
            torch.cuda.synchronize()
            t[K].append(a.steps / (time.perf_counter() - t0))
    for m in models:
        m.check_device_status()
        if not all(bool(torch.isfinite(p).all()) for p in m.parameters()):
            sys.exit("non-finite parameters after the timed steps: not reporting")
    r = {"image": [cfg["H"], cfg["W"]], "frames": len(frames), "graphs": {str(K): reports[K]["graphs"] for K in KS}}
    for K in KS:
        r["accumulate_%d_steps_per_s" % K] = _stats(t[K], a.steps)
    for K in KS[1:]:
        r["accumulate_%d_over_1" % K] = r["accumulate_%d_steps_per_s" % K]["median"] / r["accumulate_1_steps_per_s"]["median"]
    return r


PARTS = {"op": part_op, "steps": part_steps}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=16, help="timed steps per K and round: a multiple of 8")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="time limit of each child process, seconds")
    ap.add_argument("--commit", default=None, help="recorded when the tree is not a git checkout")
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default=None, choices=sorted(PARTS), help="(internal) run one measurement in this process")
    ap.add_argument("--model", default="vgg16", choices=sorted(SIZES), help="(internal) with --part")
    a = ap.parse_args()
    if a.steps < 8 or a.steps % 8:
        sys.exit("--steps: a positive multiple of 8 (whole windows at every K)")
    if a.part:
        import torch
        if not torch.cuda.is_available():
            sys.exit("grad_accum_bench needs a HIP device: nothing is measured without one")
        r = PARTS[a.part](a.model, a)
        r["device"], r["torch"] = torch.cuda.get_device_name(0), torch.__version__
        print("RESULT " + json.dumps(r))
        return
    from sgd_bench import commit
    res = {"commit": commit() or a.commit, "op": {}, "steps": {}}
    for part in ("op", "steps"):                                               # a fresh process each, under its own time limit; the first failure ends the run
        for which in ("vgg16", "resnet50_fpn"):
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--model", which] + \
                [x for k in ("replays", "rounds", "warmup", "steps", "step_rounds") for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
            try:
                p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                sys.exit("grad_accum_bench: '%s %s' ran into its limit of %d s: stopping" % (part, which, a.limit))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit("grad_accum_bench: '%s %s' failed with status %d: stopping" % (part, which, p.returncode))
            res[part][which] = json.loads(line[-1][len("RESULT "):])
    res["note"] = "one MI355X shared with other work; the graphs / the K alternate inside every round; nothing here is a pass / fail condition"
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
