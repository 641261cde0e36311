"""GPU time of the device-side training telemetry, as graph replays; recorded, never asserted.

    python tools/telemetry_bench.py [--replays 50] [--rounds 9] [--warmup 10] [--out profiles/telemetry_bench.json]

For the trainable-parameter shapes of both mirrors (model.FRCNN: VGG16, new_model.FRCNN: ResNet-50-FPN), random fp32 parameters,
gradients and born momenta, five graphs captured once each:
  (a) tensor_stats_every_1   telemetry.TensorStats.measure(), every = 1: tensor_stats_partial_kernel (12 B read per element) +
                             tensor_stats_finish_kernel + tensor_stats_advance_kernel
  (b) tensor_stats_idle_tick the same three launches on a tick that does not measure (every = 2^30, the first tick spent before the capture)
  (c) grad_norm              frcnn_grad_norm on the same table (4 B read per element): grad_norm_partial_kernel + grad_norm_finish_kernel
  (d) same_bytes_copy        one device copy that reads 6 B and writes 6 B per element: as many bytes moved as (a) reads
  (e) journal_append_8       telemetry.ScalarJournal.append with 8 float32 columns: one launch of one wave
GPU time per replay = HIP-event time around `replays` back-to-back replays / replays.  The graphs ALTERNATE inside every round (the GPU
is shared with other work), after `warmup` replays of each: median / p10 / p90 over `rounds`.  Prints one JSON line; --out writes it too."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tools")) if p not in sys.path]

from faster_rcnn_pytorch_amd import _lib  # noqa: E402
from faster_rcnn_pytorch_amd.optim import DeviceSGD  # noqa: E402
from faster_rcnn_pytorch_amd.telemetry import ScalarJournal, TensorStats  # noqa: E402
from sgd_bench import capture, commit, model_shapes, stats  # noqa: E402

HYPER = dict(lr=2e-3, momentum=0.9, weight_decay=5e-4)


def _optimizer(shapes, gen, **kw):
    ps = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).cuda()) for s in shapes]
    for p in ps:
        p.grad = (torch.randn(*p.shape, generator=gen) * 0.02).cuda()
    opt = DeviceSGD(ps, **dict(HYPER, **kw))
    opt.step()                                                   # the momenta are born: measure() reads all three streams
    return opt


def bench(shapes, a):
    gen = torch.Generator().manual_seed(0)
    busy, idle, norm = _optimizer(shapes, gen), _optimizer(shapes, gen), _optimizer(shapes, gen, skip_nonfinite=True)
    n = sum(p.numel() for p, _ in busy._rows)
    every_1, never = TensorStats(busy, every=1), TensorStats(idle, every=2 ** 30)
    never.measure()                                              # tick 0 measures; every later tick of this run does not
    src, dst = torch.empty(6 * n, dtype=torch.uint8, device="cuda").random_(0, 256), torch.empty(6 * n, dtype=torch.uint8, device="cuda")
    journal = ScalarJournal(["c%d" % c for c in range(8)], 256, "cuda")
    cols = [torch.full((1,), float(c), device="cuda") for c in range(8)]
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)          # noqa: E731

    def grad_norm():
        _lib.check(_lib.lib.frcnn_grad_norm(C.c_void_p(norm._table.data_ptr()), norm._table_bytes, len(norm._rows), norm._n_chunks,
                                            C.c_void_p(norm._gn_state.data_ptr()), None, C.c_void_p(norm._gn_work.data_ptr()), norm._gn_work_bytes, stream()),
                   "frcnn_grad_norm")
    graphs = {"tensor_stats_every_1": capture(every_1.measure), "tensor_stats_idle_tick": capture(never.measure), "grad_norm": capture(grad_norm),
              "same_bytes_copy": capture(lambda: dst.copy_(src)), "journal_append_8": capture(lambda: journal.append(cols))}
    torch.cuda.synchronize()
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
    busy_state, idle_state = every_1.read(), never.read()
    calls = 1 + a.warmup + a.rounds * a.replays                  # the capture's warm-up call, the warm-up replays, the timed replays
    if busy_state["measures"] != calls or idle_state["measures"] != 1 or idle_state["tick"] != calls + 1:
        sys.exit("the tick bookkeeping is not what the replays should have left: not reporting (%r, %r)" % (busy_state["measures"], idle_state["tick"]))
    r = {"tensors": len(shapes), "elements": n, "chunks": busy._n_chunks, "bytes_read_by_a_measuring_call": 12 * n, "bytes_read_by_grad_norm": 4 * n,
         "bytes_moved_by_the_copy": 12 * n, "measuring_calls": busy_state["measures"], "idle_calls": idle_state["tick"] - 1}
    for k in graphs:
        r[k + "_us"] = stats(t[k], a)
    med = {k: r[k + "_us"]["median"] for k in graphs}
    r["measure_over_same_bytes_copy"] = med["tensor_stats_every_1"] / med["same_bytes_copy"]
    r["measure_over_grad_norm"] = med["tensor_stats_every_1"] / med["grad_norm"]
    r["measure_read_tb_per_s"] = 12 * n / (med["tensor_stats_every_1"] * 1e-6) / 1e12
    r["copy_moved_tb_per_s"] = 12 * n / (med["same_bytes_copy"] * 1e-6) / 1e12
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
        sys.exit("telemetry_bench needs a HIP device: nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "commit": commit() or a.commit, "torch": torch.__version__, "hyper": HYPER, "models": {}}
    for which in ("vgg16", "resnet50_fpn"):
        res["models"][which] = bench(model_shapes(which), a)
        torch.cuda.empty_cache()
    res["note"] = ("one MI355X shared with other work; the graphs alternate inside every round; nothing here is a pass / fail condition; 12 B x "
                   "elements exceeds the 256 MiB Infinity Cache for both models, so the rates are HBM-side rates")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
