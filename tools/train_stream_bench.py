"""What it costs to make the number of ground-truth boxes device data; recorded, never asserted.

    python tools/train_stream_bench.py --config vgg|fpn [--frames 8] [--steps 16] [--rounds 5] [--out profiles/train_stream_bench.json]

Two measurements, each in a fresh child process under a time limit of its own (--limit seconds; a child that fails ends the run):

  targets   the two target makers alone, as graph replays, at the config's sizes (N synthetic anchors, P proposals, 8 box rows of which
            5 are live): the classic entry points frcnn_rpn_targets / frcnn_head_targets on gt[:5] -- the code path of the parent commit, which
            the library keeps -- against frcnn_rpn_targets_n / frcnn_head_targets_n on all 8 rows with the count in device memory.  GPU time
            per replay = HIP-event time around `replays` back-to-back replays / replays; the graphs alternate inside every round.
  steps     the whole training step (bench.py's synthetic frames at the config's size, DeviceSGD) over a cycle of --frames frames whose
            numbers of boxes differ, three ways, alternating inside every round, wall time per step with one synchronisation per pass:
              eager_item_slice   the frame comes as a fixed-capacity list + device count (what the device input stage hands over); the caller
                                 reads count.item() and slices before model(x, boxes, labels): a host sync per step
              graph_per_frame    parallel.GraphStep with n_frames = --frames: one A / B graph pair per resident frame (a benchmark's cycle)
              graph_one_slot     parallel.GraphStep with n_frames = 1 fed by parallel.FrameSlot.load(): one graph set, any frame

Prints one JSON line per config; --out merges it into that file under the config's name."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tools")) if p not in sys.path]

SIZES = {"vgg": dict(H=600, W=1000, N=20646, P=2000, num_classes=21, lo=0, hi=20, variant=0, label_offset=1, max_pos=32, total=128),
         "fpn": dict(H=800, W=1344, N=268569, P=1000, num_classes=91, lo=1, hi=91, variant=1, label_offset=0, max_pos=128, total=512)}
CAP = 8


def _stats(v):
    import numpy as np
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "rounds": len(v)}


def _boxes(g, n, lo, hi):
    import torch
    c = torch.rand(n, 2, generator=g) * 0.7 + 0.15
    wh = torch.rand(n, 2, generator=g) * (hi - lo) + lo
    return torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, 1)


# ------------------------------------------------------------------------------------------------ the target makers alone
def part_targets(cfg, a):
    import torch
    from faster_rcnn_pytorch_amd import ops
    from sgd_bench import capture
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    live = 5
    gt = _boxes(g, CAP, 0.08, 0.6).to(dev)
    lab = torch.randint(cfg["lo"], cfg["hi"], (CAP,), generator=g).to(dev)
    anchors = _boxes(g, cfg["N"], 0.03, 0.6)
    k = torch.arange(0, cfg["N"], 7)
    anchors[k] = (gt.cpu()[torch.randint(0, live, (k.numel(),), generator=g)] + (torch.rand(k.numel(), 4, generator=g) - 0.5) * 0.01).clamp(0, 1)
    anchors = anchors.to(dev)
    rois = _boxes(g, cfg["P"], 0.03, 0.6).to(dev)
    n_rois = torch.tensor([cfg["P"]], dtype=torch.int32, device=dev)
    n_gt, empty = torch.tensor([live], dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    gt_live, lab_live = gt[:live].contiguous(), lab[:live].contiguous()
    state = ops.philox_state(1, 1, dev)
    hk = dict(variant=cfg["variant"], label_offset=cfg["label_offset"], max_pos=cfg["max_pos"], total=cfg["total"])
    fns = {"rpn_targets_classic": lambda: ops.rpn_targets(anchors, gt_live, variant=cfg["variant"], philox_state=state),
           "rpn_targets_device_count": lambda: ops.rpn_targets(anchors, gt, variant=cfg["variant"], philox_state=state, n_gt=n_gt),
           "head_targets_classic": lambda: ops.head_targets(rois, gt_live, lab_live, n_rois=n_rois, philox_state=state, **hk),
           "head_targets_device_count": lambda: ops.head_targets(rois, gt, lab, n_rois=n_rois, philox_state=state, n_gt=n_gt, empty=empty, **hk)}
    graphs = {k_: capture(f) for k_, f in fns.items()}
    for gr in graphs.values():
        for _ in range(a.warmup):
            gr.replay()
    torch.cuda.synchronize()
    t = {k_: [] for k_ in graphs}
    for _ in range(a.rounds):
        for k_, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                gr.replay()
            e1.record()
            e1.synchronize()
            t[k_].append(1e3 * e0.elapsed_time(e1) / a.replays)
    r = {"anchors": cfg["N"], "proposals": cfg["P"], "box_rows": CAP, "live_boxes": live, "replays_per_round": a.replays}
    for k_ in graphs:
        r[k_ + "_us"] = _stats(t[k_])
    for which in ("rpn", "head"):
        old, new = r[which + "_targets_classic_us"]["median"], r[which + "_targets_device_count_us"]["median"]
        r[which + "_device_count_over_classic"] = new / old
    return r


# ------------------------------------------------------------------------------------------------ the whole step
def _frames(cfg, n_frames, dev):
    import torch
    frames = []
    for i in range(n_frames):
        g = torch.Generator().manual_seed(1000 + i)
        n = 1 + (3 * i) % CAP                                                  # 1, 4, 7, 2, 5, 8, 3, 6: every frame another count
        x = torch.randn(1, 3, cfg["H"], cfg["W"], generator=g)
        b = torch.zeros(CAP, 4)
        b[:n] = _boxes(g, n, 0.08, 0.6)
        l = torch.zeros(CAP, dtype=torch.int64)
        l[:n] = torch.randint(cfg["lo"], cfg["hi"], (n,), generator=g)
        frames.append((x.to(dev), b.to(dev), l.to(dev), torch.tensor([n], dtype=torch.int32, device=dev), n))
    return frames


def part_steps(cfg, a):
    import torch
    from faster_rcnn_pytorch_amd import parallel
    from faster_rcnn_pytorch_amd.loss import FRCNNLoss
    from faster_rcnn_pytorch_amd.optim import DeviceSGD
    if cfg["variant"] == 0:
        from faster_rcnn_pytorch_amd.model import FRCNN
    else:
        from faster_rcnn_pytorch_amd.new_model import FRCNN
    device = torch.device("cuda:0")
    frames = _frames(cfg, a.frames, device)
    crit = FRCNNLoss(None)
    hyper = dict(lr=2e-3, momentum=0.9, weight_decay=5e-4)

    def build(guard=None):
        torch.manual_seed(0)
        m = FRCNN(num_classes=cfg["num_classes"], sampling="device", seed=1).to(device)
        return m, DeviceSGD([p for p in m.parameters() if p.requires_grad], guard=guard, **hyper)

    # eager: count.item() + slice
    em, eopt = build()

    def eager_step(i):
        x, b, l, cnt, _ = frames[i % len(frames)]
        n = int(cnt.item())                                                    # the host sync the device count removes
        pred, target = em(x, [b[:n]], [l[:n]])
        loss = crit(pred, target)[0]
        eopt.zero_grad(set_to_none=True)
        loss.backward()
        eopt.step()

    # one graph pair per resident frame
    pm, popt = build()

    def per_frame_loss(f):
        x, b, l, _, n = frames[f]
        pred, target = pm(x, [b[:n]], [l[:n]])
        return crit(pred, target), pred
    pgs = parallel.GraphStep(pm, popt, per_frame_loss, len(frames), device, **pm.graph_stages()).capture()

    # one slot, one graph set
    slot = parallel.FrameSlot((cfg["H"], cfg["W"]), CAP, device)
    sm, sopt = build(guard=slot.empty)

    def slot_loss(f):
        pred, target = sm(slot.x, [slot.boxes], [slot.labels], n_gt=slot.n_gt, empty=slot.empty)
        return crit(pred, target), pred
    slot.load(*frames[0][:4])
    sgs = parallel.GraphStep(sm, sopt, slot_loss, 1, device, **sm.graph_stages()).capture()

    def slot_step(i):
        slot.load(*frames[i % len(frames)][:4])
        sgs.step(i)
    ways = {"eager_item_slice": eager_step, "graph_per_frame": pgs.step, "graph_one_slot": slot_step}
    for fn in ways.values():
        for i in range(a.warmup):
            fn(i)
    torch.cuda.synchronize()
    t = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():                                             # alternating: every round times each way
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                fn(i)
            torch.cuda.synchronize()
            t[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
    for m in (em, pm, sm):
        m.check_device_status()
        if not all(bool(torch.isfinite(p).all()) for p in m.parameters()):
            sys.exit("non-finite parameters after the timed steps: not reporting")
    r = {"frames": len(frames), "boxes_per_frame": [f[4] for f in frames], "box_rows": CAP, "steps_per_round": a.steps,
         "graphs": {"graph_per_frame": pgs.report()["graphs"], "graph_one_slot": sgs.report()["graphs"]}}
    for k in ways:
        r[k + "_ms_per_step"] = _stats(t[k])
    r["one_slot_over_per_frame"] = r["graph_one_slot_ms_per_step"]["median"] / r["graph_per_frame_ms_per_step"]["median"]
    r["one_slot_over_eager"] = r["graph_one_slot_ms_per_step"]["median"] / r["eager_item_slice_ms_per_step"]["median"]
    return r


PARTS = {"targets": part_targets, "steps": part_steps}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="vgg", choices=sorted(SIZES))
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=16, help="timed steps per way and round (a multiple of --frames times every frame equally)")
    ap.add_argument("--replays", type=int, default=50, help="graph replays per round (the target makers alone)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--limit", type=int, default=420, help="time limit of each child process, seconds")
    ap.add_argument("--commit", default=None, help="recorded when the tree is not a git checkout")
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default=None, choices=sorted(PARTS), help="(internal) run one measurement in this process")
    a = ap.parse_args()
    if a.frames < 8:
        sys.exit("--frames: at least 8 (the cycle must hold frames whose numbers of boxes differ)")
    cfg = SIZES[a.config]
    if a.part:
        import torch
        if not torch.cuda.is_available():
            sys.exit("train_stream_bench needs a HIP device: nothing is measured without one")
        r = PARTS[a.part](cfg, a)
        r["device"], r["torch"] = torch.cuda.get_device_name(0), torch.__version__
        print("RESULT " + json.dumps(r))
        return
    from sgd_bench import commit
    res = {"config": a.config, "image": [cfg["H"], cfg["W"]], "commit": commit() or a.commit}
    for part in ("targets", "steps"):                                          # a fresh process each, under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part] + [x for k in ("config", "frames", "steps", "replays", "rounds", "warmup")
                                                                              for x in ("--" + k, str(getattr(a, k)))]
        try:
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.exit("train_stream_bench: '%s' ran into its limit of %d s: stopping" % (part, a.limit))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit("train_stream_bench: '%s' failed with status %d: stopping" % (part, p.returncode))
        res[part] = json.loads(line[-1][len("RESULT "):])
    res["note"] = "one MI355X shared with other work; the ways alternate inside every round; nothing here is a pass / fail condition"
    print(json.dumps(res))
    if a.out:
        merged = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                merged = json.load(f)
        merged[a.config] = res
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
