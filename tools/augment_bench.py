"""GPU time of the device-side photometric distortion and zoom-out (transforms.photometric_distort / zoom_out, csrc/photometric.hip),
recorded, never asserted.

    python tools/augment_bench.py [--replays 200] [--rounds 9] [--warmup 20] [--cpu-reps 3] [--out profiles/augment_bench.json]

Two seeded uint8 frames, 375 x 500 and 1333 x 1333; a full four-op plan with contrast in third place (both passes do work); a zoom-out
of scale 1.5 with 8 boxes.  Per frame and per function:
  * the call captured once into a graph; GPU time per call = HIP-event time around `replays` back-to-back replays / replays, once per
    round, after `warmup` replays: median / p10 / p90 over `rounds`.
  * a same-bytes device copy measured the same way in the same run: one dense device-to-device copy that moves as many bytes in total
    (read + written) as the function must -- photometric reads the frame twice and writes it once (3 F bytes: a copy of 1.5 F), zoom-out
    reads the frame twice and writes the canvas once (2 F + C bytes: a copy of F + C / 2) -- and the function's time as a fraction
    of it (copy time / function time: 1.0 means as fast as the copy).
  * per-kernel GPU time of eager calls from the in-library profiler (median).
  * the wall time of the CPU restatement (tests/photometric_ref.py, numpy), and of Pillow where it is installed (ImageEnhance / HSV
    round trip in the plan's order; Image.new + paste with ImageStat's median).
The device result is compared with the restatement (exactly) before anything is timed.  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

from faster_rcnn_pytorch_amd import _lib, transforms as T  # noqa: E402
import photometric_ref as R  # noqa: E402

ORDER, FACTORS = (2, 3, 1, 0), {0: 1.21, 1: 0.74, 2: 1.38, 3: -0.043}


def graph_us(fn, replays, rounds, warmup):
    """fn captured once; microseconds of GPU time per replay: median / p10 / p90 over the rounds."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            g.replay()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / replays)
    return {"median": float(np.median(out)), "p10": float(np.percentile(out, 10)), "p90": float(np.percentile(out, 90)),
            "replays_per_round": replays, "rounds": rounds}


def copy_us(total_bytes, a):
    n = int(total_bytes) // 2
    src, dst = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    return dict(graph_us(lambda: dst.copy_(src), a.replays, a.rounds, a.warmup), bytes_copied=n)


def kernel_us(fn, calls):
    _lib.prof_reset()
    _lib.prof_enable(True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    return {k: float(np.median(v)) * 1e3 for k, v in sorted(_lib.prof_samples().items())}


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def pillow_fns(img, plan_order, new_hw, top_left):
    try:
        from PIL import Image, ImageEnhance, ImageStat
    except ImportError:
        return None, None
    im = Image.fromarray(img, "RGB")

    def photometric():
        x = im
        for op in plan_order:
            if op == R.HUE:
                h, s, v = x.convert("HSV").split()
                hh = np.array(h, dtype=np.uint8)
                hh += np.uint8(R.hue_shift(FACTORS[op]))
                x = Image.merge("HSV", (Image.fromarray(hh, "L"), s, v)).convert("RGB")
            else:
                x = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](x).enhance(FACTORS[op])
        return x

    def zoom():
        c = Image.new("RGB", (new_hw[1], new_hw[0]), tuple(ImageStat.Stat(im).median))
        c.paste(im, (top_left[1], top_left[0]))
        return c
    return photometric, zoom


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_bench needs a HIP device: nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "plan_order": list(ORDER), "factors": {str(k): v for k, v in FACTORS.items()}, "frames": {}}
    plan = T.photometric_plan(ORDER, FACTORS)
    d_plan = torch.from_numpy(plan).cuda()
    for h, w in ((375, 500), (1333, 1333)):
        rng = np.random.RandomState(h)
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        x1, y1 = rng.uniform(0, w * 0.6, 8), rng.uniform(0, h * 0.6, 8)
        boxes = np.stack([x1, y1, x1 + rng.uniform(20, w * 0.4, 8), y1 + rng.uniform(20, h * 0.4, 8)], 1).astype(np.float32)
        new_hw, top_left = (int(1.5 * h), int(1.5 * w)), (h // 5, w // 7)
        d_img, d_boxes, d_out = torch.from_numpy(img).cuda(), torch.from_numpy(boxes).cuda(), torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        run_p = lambda: T.photometric_distort(d_img, d_plan, out=d_out)          # noqa: E731
        run_z = lambda: T.zoom_out(d_img, d_boxes, new_hw, top_left)             # noqa: E731
        ref_p, (ref_c, ref_b) = R.apply_plan(img, plan), R.zoom_out(img, boxes, new_hw, top_left)
        canvas, bo = run_z()
        if not (np.array_equal(run_p().cpu().numpy(), ref_p) and np.array_equal(canvas.cpu().numpy(), ref_c) and np.array_equal(bo.cpu().numpy(), ref_b)):
            sys.exit("the device result differs from the restatement at %d x %d: not timing a wrong result" % (h, w))
        F, Cv = img.nbytes, ref_c.nbytes
        r = {"frame_bytes": F, "canvas_hw": list(new_hw), "canvas_bytes": Cv, "equal_to_cpu_restatement": True}
        r["photometric_graph_replay_us"] = graph_us(run_p, a.replays, a.rounds, a.warmup)
        r["photometric_same_bytes_copy_us"] = copy_us(3 * F, a)
        r["photometric_fraction_of_copy"] = r["photometric_same_bytes_copy_us"]["median"] / r["photometric_graph_replay_us"]["median"]
        r["zoom_out_graph_replay_us"] = graph_us(run_z, a.replays, a.rounds, a.warmup)
        r["zoom_out_same_bytes_copy_us"] = copy_us(2 * F + Cv, a)
        r["zoom_out_fraction_of_copy"] = r["zoom_out_same_bytes_copy_us"]["median"] / r["zoom_out_graph_replay_us"]["median"]
        r["kernel_us_eager"] = kernel_us(lambda: (run_p(), run_z()), 50)
        pil_p, pil_z = pillow_fns(img, ORDER, new_hw, top_left)
        r["cpu_restatement_wall_ms"] = {"photometric": wall_ms(lambda: R.apply_plan(img, plan), a.cpu_reps),
                                        "zoom_out": wall_ms(lambda: R.zoom_out(img, boxes, new_hw, top_left), a.cpu_reps), "reps": a.cpu_reps}
        r["pillow_wall_ms"] = None if pil_p is None else {"photometric": wall_ms(pil_p, a.cpu_reps), "zoom_out": wall_ms(pil_z, a.cpu_reps), "reps": a.cpu_reps}
        res["frames"]["%dx%d" % (h, w)] = r
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
