"""GPU time of one optimizer update with the weight average fused in, against the two-pass sequence, as graph replays; recorded, never
asserted.

    python tools/ema_bench.py [--replays 50] [--rounds 9] [--warmup 10] [--out profiles/ema_bench.json]

For the trainable-parameter shapes of both mirrors (model.FRCNN: VGG16, new_model.FRCNN: ResNet-50-FPN), random fp32 parameters and
gradients, lr 2e-3, momentum 0.9, weight decay 5e-4 (main.py:58-61), decay 0.9998 with warm-up, each graph captured once on its own
copy of the tensors:
  (a) device_sgd          optim.DeviceSGD alone: sgd_update_kernel<false, false> + sgd_born_kernel                       20 B per element
  (b) fused               optim.DeviceSGD(ema=): sgd_update_kernel<false, true> + sgd_born_kernel + ema_advance_kernel   28 B per element
  (c) two_pass            optim.DeviceSGD, then WeightEMA.update(): (a) + ema_update_kernel + ema_advance_kernel         32 B per element
  (d) copy_28             one device copy that moves the bytes of (b): 14 B read + 14 B written per element (a flat fp32 buffer of 3.5 n)
  (e) swap                one WeightEMA.swap(): ema_swap_kernel                                                          16 B per element
GPU time per replay = HIP-event time around `replays` back-to-back replays / replays.  The graphs ALTERNATE inside every round (the GPU
is shared with other work), after `warmup` replays of each: median / p10 / p90 over `rounds`.  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tools")) if p not in sys.path]

from faster_rcnn_pytorch_amd.optim import DeviceSGD, WeightEMA  # noqa: E402
from sgd_bench import capture, commit, model_shapes, stats  # noqa: E402

HYPER = dict(lr=2e-3, momentum=0.9, weight_decay=5e-4)
EMA = dict(decay=0.9998, warmup=True)
BYTES = {"device_sgd": 20, "fused": 28, "two_pass": 32, "copy_28": 28, "swap": 16}


def bench(shapes, a):
    gen = torch.Generator().manual_seed(0)
    init = [torch.randn(*s, generator=gen) * 0.1 for s in shapes]
    grad = [torch.randn(*s, generator=gen) * 0.02 for s in shapes]
    sets = []
    for _ in range(3):
        ps = [torch.nn.Parameter(t.cuda()) for t in init]
        for p, g in zip(ps, grad):
            p.grad = g.cuda()
        sets.append(ps)
    n = sum(p.numel() for p in sets[0])
    alone = DeviceSGD(sets[0], **HYPER)
    ema_f = WeightEMA(sets[1], **EMA)
    fused = DeviceSGD(sets[1], ema=ema_f, **HYPER)
    ema_t = WeightEMA(sets[2], **EMA)
    first = DeviceSGD(sets[2], **HYPER)
    ema_s = WeightEMA(sets[0], **EMA)                            # the swap has an average of its own: (b) and (c) must never see swapped set
    src, dst = torch.randn(n * 7 // 2, device="cuda"), torch.empty(n * 7 // 2, device="cuda")

    def two_pass():
        first.launch()
        ema_t.update()
    for o in (alone, fused, first):
        o.push_hyper()
        o.prepare()
    graphs = {"device_sgd": capture(alone.launch), "fused": capture(fused.launch), "two_pass": capture(two_pass),
              "copy_28": capture(lambda: dst.copy_(src)), "swap": capture(ema_s.swap)}
    torch.cuda.synchronize()                                     # each capture's warm-up call was one update (one swap)
    for g in graphs.values():
        for _ in range(a.warmup + a.warmup % 2):                 # an even number: the swap graph ends where it began
            g.replay()
    torch.cuda.synchronize()
    t = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():                              # alternating: every round times each graph
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays + (a.replays % 2 if k == "swap" else 0)):
                g.replay()
            e1.record()
            e1.synchronize()
            t[k].append(1e3 * e0.elapsed_time(e1) / (a.replays + (a.replays % 2 if k == "swap" else 0)))
    r = {"tensors": len(shapes), "elements": n, "chunks": fused._n_chunks, "bytes_per_element": BYTES}
    for k in graphs:
        r[k + "_us"] = stats(t[k], a)
        r[k + "_tb_per_s"] = BYTES[k] * n / (r[k + "_us"]["median"] * 1e-6) / 1e12
    med = {k: r[k + "_us"]["median"] for k in graphs}
    r["fused_minus_device_sgd_us"] = med["fused"] - med["device_sgd"]
    r["two_pass_minus_device_sgd_us"] = med["two_pass"] - med["device_sgd"]
    r["fused_over_two_pass"] = med["fused"] / med["two_pass"]
    r["fused_over_copy_28"] = med["fused"] / med["copy_28"]
    sf, st = ema_f.stats(), ema_t.stats()
    r["fused_ema_stats"], r["two_pass_ema_stats"] = sf, st
    if ema_s.stats()["swapped"] != 1 or sf["refused"] or st["refused"]:    # the capture's one eager swap; the replayed ones come in pairs
        sys.exit("the swap graph did not end where it began, or an update was refused: not reporting")
    if not all(bool(torch.isfinite(p).all()) for ps in sets for p in ps) or not all(bool(torch.isfinite(e).all()) for e in ema_f.shadow + ema_t.shadow):
        sys.exit("non-finite parameters or averages after the timed replays: not reporting")
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--commit", default=None, help="recorded when the tree is not a git checkout")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ema_bench needs a HIP device: nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "commit": commit() or a.commit, "torch": torch.__version__, "hyper": HYPER, "ema": EMA, "models": {}}
    for which in ("vgg16", "resnet50_fpn"):
        res["models"][which] = bench(model_shapes(which), a)
        torch.cuda.empty_cache()
    res["note"] = "one MI355X shared with other work; the graphs alternate inside every round; nothing here is a pass / fail condition"
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
