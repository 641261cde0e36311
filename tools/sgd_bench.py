"""GPU time of one optimizer update as a graph replay, recorded, never asserted.

    python tools/sgd_bench.py [--replays 50] [--rounds 9] [--warmup 10] [--out profiles/sgd_bench.json]

For the trainable-parameter shapes of both mirrors (model.FRCNN: VGG16, new_model.FRCNN: ResNet-50-FPN), random fp32 parameters and
gradients, lr 2e-3, momentum 0.9, weight decay 5e-4 (main.py:58-61), three graphs captured once each:
  * optim.DeviceSGD          the library launch (csrc/sgd.hip: sgd_update_kernel + sgd_born_kernel)
  * torch.optim.SGD(fused=True)   its step(), captured the same way, on its own copy of the tensors
  * a same-bytes device copy      one dense device-to-device copy moving 20 B per element in total (12 read + 8 written by an update)
GPU time per replay = HIP-event time around `replays` back-to-back replays / replays.  The three graphs ALTERNATE inside every round
(the GPU is shared with other work), after `warmup` replays of each: median / p10 / p90 over `rounds`.  Before anything is timed one
update of each optimizer is compared (the largest absolute difference is recorded; the bit-for-bit reference is torch on the CPU,
tests/test_gpu_sgd.py).  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT,) if p not in sys.path]

from faster_rcnn_pytorch_amd.optim import DeviceSGD  # noqa: E402

HYPER = dict(lr=2e-3, momentum=0.9, weight_decay=5e-4)


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:                                            # noqa: BLE001 -- not a git checkout: the caller records the commit
        return None


def model_shapes(which):
    if which == "vgg16":
        from faster_rcnn_pytorch_amd.model import FRCNN
        m = FRCNN(num_classes=21, sampling="device")
    else:
        from faster_rcnn_pytorch_amd.new_model import FRCNN
        m = FRCNN(num_classes=91, sampling="device")
    return [tuple(p.shape) for p in m.parameters() if p.requires_grad]


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def stats(v, a):
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "replays_per_round": a.replays,
            "rounds": a.rounds}


def bench(shapes, a):
    gen = torch.Generator().manual_seed(0)
    init = [torch.randn(*s, generator=gen) * 0.1 for s in shapes]
    grad = [torch.randn(*s, generator=gen) * 0.02 for s in shapes]
    sets = []
    for _ in range(2):
        ps = [torch.nn.Parameter(t.cuda()) for t in init]
        for p, g in zip(ps, grad):
            p.grad = g.cuda()
        sets.append(ps)
    ours, theirs = DeviceSGD(sets[0], **HYPER), torch.optim.SGD(sets[1], fused=True, **HYPER)
    n = sum(p.numel() for p in sets[0])
    src, dst = torch.empty(10 * n, dtype=torch.uint8, device="cuda").random_(0, 256), torch.empty(10 * n, dtype=torch.uint8, device="cuda")
    ours.push_hyper()
    ours.prepare()
    graphs = {"device_sgd": capture(ours.launch), "torch_fused_sgd": capture(theirs.step), "same_bytes_copy": capture(lambda: dst.copy_(src))}
    torch.cuda.synchronize()                                     # each capture's warm-up call was one update of each optimizer
    diff = max(float((x.detach() - y.detach()).abs().max()) for x, y in zip(*sets))
    for g in graphs.values():
        for _ in range(a.warmup):
            g.replay()
    torch.cuda.synchronize()
    t = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():                              # alternating: every round times each of the three
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                g.replay()
            e1.record()
            e1.synchronize()
            t[k].append(1e3 * e0.elapsed_time(e1) / a.replays)
    r = {"tensors": len(shapes), "elements": n, "bytes_moved_per_update": 20 * n, "max_abs_diff_vs_torch_fused_after_one_update": diff}
    for k in graphs:
        r[k + "_us"] = stats(t[k], a)
    r["device_sgd_over_torch_fused"] = r["device_sgd_us"]["median"] / r["torch_fused_sgd_us"]["median"]
    r["device_sgd_fraction_of_copy"] = r["same_bytes_copy_us"]["median"] / r["device_sgd_us"]["median"]
    r["device_sgd_tb_per_s"] = 20 * n / (r["device_sgd_us"]["median"] * 1e-6) / 1e12
    if not all(bool(torch.isfinite(p).all()) for ps in sets for p in ps):
        sys.exit("non-finite parameters after the timed replays: not reporting")
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sgd_bench needs a HIP device: nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "commit": commit(), "torch": torch.__version__, "hyper": HYPER, "models": {}}
    for which in ("vgg16", "resnet50_fpn"):
        res["models"][which] = bench(model_shapes(which), a)
        torch.cuda.empty_cache()
    res["note"] = "one MI355X shared with other work; the three graphs alternate inside every round; nothing here is a pass / fail condition"
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
