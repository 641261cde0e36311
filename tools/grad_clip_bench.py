"""GPU time of one optimizer update with and without device-side gradient clipping, as graph replays; recorded, never asserted.

    python tools/grad_clip_bench.py [--replays 50] [--rounds 9] [--warmup 10] [--out profiles/grad_clip_bench.json]

For the trainable-parameter shapes of both mirrors (model.FRCNN: VGG16, new_model.FRCNN: ResNet-50-FPN), random fp32 parameters and
gradients, lr 2e-3, momentum 0.9, weight decay 5e-4 (main.py:58-61), max_grad_norm 1.0, four graphs captured once each:
  (a) device_sgd            optim.DeviceSGD, the plain update: sgd_update_kernel<false> + sgd_born_kernel
  (b) device_sgd_clip       optim.DeviceSGD(max_grad_norm=1.0, skip_nonfinite=True): grad_norm_partial_kernel + grad_norm_finish_kernel +
                            sgd_update_kernel<true> + sgd_born_kernel.  The partial kernel's loads use the default cache policy (the only
                            variant built: no non-temporal build switch is kept), the update's gradient load stays non-temporal.
  (c) torch_clip_fused_sgd  torch.nn.utils.clip_grad_norm_(foreach=True) + torch.optim.SGD(fused=True).step(), captured the same way, on
                            its own copy of the tensors (it rewrites the gradients)
  (d) gradient_read         one device pass that only READS as many bytes as the gradients have (a sum over one flat fp32 buffer)
GPU time per replay = HIP-event time around `replays` back-to-back replays / replays.  The graphs ALTERNATE inside every round (the GPU
is shared with other work), after `warmup` replays of each: median / p10 / p90 over `rounds`.  Before anything is timed the norm the
device measured (binary64 sum in a fixed order) is compared with the one clip_grad_norm_ returns (fp32 norm of per-tensor fp32 norms)
on the same gradients; the difference is recorded.  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tools")) if p not in sys.path]

from faster_rcnn_pytorch_amd.optim import DeviceSGD  # noqa: E402
from sgd_bench import capture, commit, model_shapes, stats  # noqa: E402

HYPER = dict(lr=2e-3, momentum=0.9, weight_decay=5e-4)
MAX_NORM = 1.0


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
    plain = DeviceSGD(sets[0], **HYPER)
    clip = DeviceSGD(sets[1], max_grad_norm=MAX_NORM, skip_nonfinite=True, **HYPER)
    theirs = torch.optim.SGD(sets[2], fused=True, **HYPER)
    flat = torch.randn(n, device="cuda")
    sink = torch.zeros((), device="cuda")

    def torch_step():
        torch.nn.utils.clip_grad_norm_(sets[2], MAX_NORM, foreach=True)
        theirs.step()

    def read_only():
        torch.sum(flat, dim=(0,), out=sink)
    torch_norm = float(torch.nn.utils.clip_grad_norm_(sets[2], float("inf"), foreach=True))     # coefficient 1: the gradients stay as they are
    for o in (plain, clip):
        o.push_hyper()
        o.prepare()
    graphs = {"device_sgd": capture(plain.launch), "device_sgd_clip": capture(clip.launch), "torch_clip_fused_sgd": capture(torch_step),
              "gradient_read": capture(read_only)}
    torch.cuda.synchronize()                                     # each capture's warm-up call was one update of each optimizer
    st = clip.grad_stats()
    for g in graphs.values():
        for _ in range(a.warmup):
            g.replay()
    torch.cuda.synchronize()
    t = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():                              # alternating: every round times each graph
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                g.replay()
            e1.record()
            e1.synchronize()
            t[k].append(1e3 * e0.elapsed_time(e1) / a.replays)
    r = {"tensors": len(shapes), "elements": n, "gradient_bytes": 4 * n, "chunks": clip._n_chunks, "max_grad_norm": MAX_NORM,
         "device_norm": st["norm"], "device_sumsq": st["sumsq"], "device_coef": st["coef"], "torch_norm_fp32": torch_norm,
         "norm_relative_difference": abs(st["norm"] - torch_norm) / torch_norm,
         "norm_difference_in_fp32_ulps": abs(int(np.float32(st["norm"]).view(np.int32)) - int(np.float32(torch_norm).view(np.int32)))}
    for k in graphs:
        r[k + "_us"] = stats(t[k], a)
    med = {k: r[k + "_us"]["median"] for k in graphs}
    r["clip_minus_plain_us"] = med["device_sgd_clip"] - med["device_sgd"]
    r["torch_minus_plain_us"] = med["torch_clip_fused_sgd"] - med["device_sgd"]
    r["clip_minus_plain_over_gradient_read"] = r["clip_minus_plain_us"] / med["gradient_read"]
    r["gradient_read_tb_per_s"] = 4 * n / (med["gradient_read"] * 1e-6) / 1e12
    end = clip.grad_stats()
    r["clip_steps_counted"], r["clip_steps_skipped"] = end["steps"], end["skipped_steps"]
    if not all(bool(torch.isfinite(p).all()) for ps in sets for p in ps):
        sys.exit("non-finite parameters after the timed replays: not reporting")
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
        sys.exit("grad_clip_bench needs a HIP device: nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "commit": commit() or a.commit, "torch": torch.__version__, "hyper": HYPER,
           "partial_kernel_loads": "default cache policy (no non-temporal variant is built)", "models": {}}
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
