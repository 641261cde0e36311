"""GPU time of the device-side resize + crop (transforms.crop, csrc/crop.hip), recorded, never asserted.

    python tools/crop_bench.py [--replays 200] [--rounds 9] [--warmup 20] [--cpu-reps 3] [--out profiles/crop_bench.json]

One seeded 480 x 640 uint8 frame with 24 boxes, resized to 600 x 800 (RandomResize([600])), and three regions of
RandomSizeCrop(384, 600): the smallest (384 x 384), the largest (600 x 600) and a seeded draw; plus a plain 384 x 384 crop of the
frame itself (the copy path).  Per region:
  * the call captured once into a graph; GPU time per call = HIP-event time around `replays` back-to-back replays / replays, once per
    round, after `warmup` replays: median / p10 / p90 over `rounds`.
  * a same-bytes device copy measured the same way in the same run: one dense device-to-device copy that moves as many bytes in total
    (read + written) as the call must at least -- the source rows and columns the region's windows reach, read once, and the region
    written once -- and the call's time as a fraction of it (copy time / call time: 1.0 means as fast as the copy).
  * per-kernel GPU time of eager calls from the in-library profiler (median).
  * the wall time of the CPU restatement (tests/crop_ref.py), which resizes the WHOLE frame and slices, and of Pillow where it is installed.
The device result is compared with the restatement (exactly) before anything is timed.  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import random
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")) if p not in sys.path]

from faster_rcnn_pytorch_amd import transforms as T  # noqa: E402
import crop_ref as R  # noqa: E402
from augment_bench import graph_us, kernel_us, wall_ms  # noqa: E402


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:                                            # noqa: BLE001 -- not a git checkout: the caller records the commit
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("crop_bench needs a HIP device: nothing is measured without one")
    img, boxes, labels, crowd = R.full_frame()
    h, w = img.shape[:2]
    hw1 = T.get_size((w, h), 600, None)
    drawn = T.draw_random_size_crop(hw1[0], hw1[1], 384, 600, random.Random(384600))
    d_img, d_b, d_l, d_c = (torch.from_numpy(x).cuda() for x in (img, boxes, labels, crowd))
    res = {"device": torch.cuda.get_device_name(0), "commit": commit(), "frame_hw": [h, w], "resize_hw": list(hw1), "boxes": len(boxes), "regions": {}}
    for name, resize_hw, region in (("min_384x384", hw1, (108, 208, 384, 384)), ("max_600x600", hw1, (0, 100, 600, 600)),
                                    ("drawn", hw1, drawn), ("plain_384x384_no_resize", None, (48, 128, 384, 384))):
        run = lambda: T.crop(d_img, d_b, d_l, region, resize_hw, iscrowd=d_c)                  # noqa: E731
        ref = R.crop_ref(img, boxes, labels, crowd, resize_hw, region)
        out = run()
        n = int(out.count.item())
        if not (n == len(ref[1]) and np.array_equal(out.img_u8.cpu().numpy(), ref[0]) and np.array_equal(out.boxes[:n].cpu().numpy(), ref[1])
                and np.array_equal(out.area[:n].cpu().numpy(), ref[3])):
            sys.exit("the device result differs from the restatement at region %s: not timing a wrong result" % (region,))
        H1, W1 = resize_hw or (h, w)
        i, j, ch, cw = region
        src_bytes = int(np.ceil(ch * h / H1 + 2) * np.ceil(cw * w / W1 + 2)) * 3 if resize_hw else ch * cw * 3
        total = src_bytes + ch * cw * 3
        ncopy = total // 2
        src, dst = torch.randint(0, 256, (ncopy,), dtype=torch.uint8, device="cuda"), torch.empty(ncopy, dtype=torch.uint8, device="cuda")
        r = {"region": list(region), "resize_hw": list(resize_hw) if resize_hw else None, "boxes_kept": n, "least_bytes_moved": total,
             "equal_to_cpu_restatement": True}
        r["graph_replay_us"] = graph_us(run, a.replays, a.rounds, a.warmup)
        r["same_bytes_copy_us"] = dict(graph_us(lambda: dst.copy_(src), a.replays, a.rounds, a.warmup), bytes_copied=ncopy)
        r["fraction_of_copy"] = r["same_bytes_copy_us"]["median"] / r["graph_replay_us"]["median"]
        r["kernel_us_eager"] = kernel_us(run, 50)
        r["cpu_restatement_wall_ms"] = {"resize_whole_frame_then_slice": wall_ms(lambda: R.crop_ref(img, boxes, labels, crowd, resize_hw, region), a.cpu_reps),
                                        "reps": a.cpu_reps}
        try:
            from PIL import Image
            pil = Image.fromarray(img, "RGB")
            r["pillow_wall_ms"] = wall_ms(lambda: (pil.resize((W1, H1), Image.BILINEAR) if resize_hw else pil).crop((j, i, j + cw, i + ch)).load(), a.cpu_reps)
        except ImportError:
            r["pillow_wall_ms"] = None
        res["regions"][name] = r
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
