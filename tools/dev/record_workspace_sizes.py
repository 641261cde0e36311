#!/usr/bin/env python
"""Records what every workspace-size function of libfrcnn_hip.so answers on a grid of arguments, into tests/golden/workspace_sizes.json.
tests/test_workspace_sizes_host.py replays the table against the library under test, so the table is recorded from a build of the commit
whose sizes are the reference (before a change to the host-side layout code), never from the code under test:

    python tools/dev/record_workspace_sizes.py [path/to/libfrcnn_hip.so] [out.json]

ctypes only, no GPU: the sizes that depend on the CU count (OP_RPN_CONV_F32, frcnn_conv3x3_f32_workspace and what is sized through it)
come out with the library's no-device fallback of 256 CUs, which is also the MI355X's count.

A row is [function, [arguments], bytes]; an argument that is a list is passed as an int32 array.  "sig" gives each function's argument
types: i = int, q = int64_t, I = const int32_t *."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIG = {
    "frcnn_workspace_bytes": "iqq",
    "frcnn_rpn_conv3x3_f32_workspace": "IIii",
    "frcnn_gemm_nt_f32_workspace": "",
    "frcnn_conv3x3_c3_wgrad_workspace": "ii",
    "frcnn_conv3x3_f32_workspace": "IIiii",
    "frcnn_conv3x3_f32_xt_floats": "IIii",
    "frcnn_conv3x3_f32_relu_bits_words": "IIii",
    "frcnn_conv3x3_f32_u_floats": "IIiii",
    "frcnn_ms_roi_align_bwd_workspace": "IIiiq",
    "frcnn_mosaic_workspace": "Iii",
    "frcnn_photometric_workspace": "ii",
    "frcnn_zoom_out_workspace": "iiii",
    "frcnn_resize_crop_workspace": "iiiiii",
    "frcnn_grad_norm_workspace_bytes": "i",
    "frcnn_tensor_stats_workspace_bytes": "ii",
}

# limits and switches of the layout code (csrc): a size on each side of every one
NMS_CASCADE_MIN, SS_MIN_N, DM_MAX_CAND, DET_MAX_P, DET_MAX_C, RPN_MAX_G = 16384, 4096, 2048, 2048, 256, 4096
EVAL_MAX_P, EVAL_MAX_C, EVAL_MAX_G = 2048, 256, 1024
N_VGG, N_FPN = 20646, 268569                                  # anchors at 600 x 1000 (stride 16, 9 per cell) and of the FPN at 800 x 1344
FPN = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]  # level shapes at 800 x 1344
VGG = [(600, 1000, 64, 64), (300, 500, 64, 128), (300, 500, 128, 128), (150, 250, 128, 256), (150, 250, 256, 256), (75, 125, 256, 512),
       (75, 125, 512, 512), (37, 62, 512, 512)]               # the VGG16 layers past conv1_1 at 600 x 1000: H, W, Cin, Cout


def hw(n1, n2):
    return (n1 << 32) | n2


def op_rows():
    g = []                                                     # (op, n1, n2)
    edge = lambda v: [v - 1, v, v + 1]                         # noqa: E731
    for n in [1, 2, 300, 2000, 6000, 12000, N_VGG, 65536, N_FPN, (1 << 22)] + edge(SS_MIN_N):
        g.append((1, n, 0))                                    # TOPK
    for k in [1, 63, 64, 65, 300, 2000, 4000, 6000, 12000, 65536] + edge(NMS_CASCADE_MIN):
        g.append((2, k, 0))                                    # NMS
    for n, k in [(N_VGG, 12000), (N_VGG, 6000), (N_FPN, 4000), (N_FPN, 2000), (65536, 65536), (4096, 300), (1, 1), (300, 12000), (4095, 4095),
                 (4097, 4097), (NMS_CASCADE_MIN + 1, NMS_CASCADE_MIN + 1), (NMS_CASCADE_MIN - 1, NMS_CASCADE_MIN), (N_FPN, NMS_CASCADE_MIN + 1)]:
        g.append((3, n, k))                                    # REGION_PROPOSAL
    for n, gt in [(N_VGG, 1), (N_VGG, 56), (N_FPN, 1), (N_FPN, 100), (1, 1), (1023, 1), (1025, 33), (N_VGG, RPN_MAX_G), (N_VGG, RPN_MAX_G + 1)]:
        g.append((4, n, gt))                                   # RPN_TARGETS
    for n in [1, 2000, 2056, 1 << 20]:
        g.append((5, n, 0))                                    # HEAD_TARGETS
    for a, b in [((375, 500), (600, 800)), ((480, 640), (800, 1067)), ((1, 1), (1, 1)), ((1, 1), (600, 1000)), ((1333, 2000), (600, 900)),
                 ((333, 500), (600, 901)), ((0, 5), (5, 5)), ((5, 5), (5, 0))]:
        g.append((6, hw(*a), hw(*b)))                          # PREPROCESS
    for c in [1, 256, 512, 0]:
        g.append((7, c, 0))                                    # HEAD_BWD
    g += [(8, 0, 0), (8, 7, 9), (9, 0, 0), (9, 7, 9)]          # RPN_CONV, RPN_CONV_WGRAD: no arguments
    for c in [1, 64, 128, 256, 512, 4096, 0, 4097]:
        g.append((10, c, 0))                                   # RPN_CONV_F32 (CU count: 256)
    for p, c in [(300, 21), (1000, 91), (128, 21), (1, 2), (DET_MAX_P, DET_MAX_C), (DET_MAX_P, 2), (1, DET_MAX_C), (0, 21), (DET_MAX_P + 1, 21),
                 (300, 1), (300, DET_MAX_C + 1)]:
        g.append((11, p, c))                                   # DETECT
    dg = [(6000, 64), (300 * 20, 100), (100 * 90, 1024), (1, 1), (255 * EVAL_MAX_P, EVAL_MAX_G), (63, 1), (64, 2), (65, 3), (0, 1), (1, 0),
          (255 * EVAL_MAX_P + 1, 1), (100, EVAL_MAX_G + 1)]
    for op in (12, 13, 15):                                    # EVAL, COCO_EVAL, COCO_EVAL_POOLED
        g += [(op, d, gt) for d, gt in dg]
    for n1, n2 in [(0, 0), (1, 1), (8 * 100000, 8 * 5000), (2 * 4096, 2 * 4952), (1000, 31), (1000, 32), (1000, 33), (4095, 255), (4096, 256),
                   ((1 << 31) - 4097, (1 << 30) - 1), ((1 << 31) - 4096, 1), (1, 1 << 30)]:
        g.append((14, n1, n2))                                 # EVAL_MERGE
    for cap, c in [(100, 21), (300, 91), (0, 2), (1, 2)] + [(v, 21) for v in edge(DM_MAX_CAND)] + [(DM_MAX_CAND, 256), (1 << 20, 256), (100, 1),
                                                                                                     (100, 257)]:
        g.append((16, cap, c))                                 # DETECT_MERGE
    for op in range(1, 17):                                    # refusals: a negative argument
        g += [(op, -1, 1), (op, 1, -1)]
    g += [(99, 1, 1), (0, 1, 1), (17, 1, 1)]                   # no such op
    return [("frcnn_workspace_bytes", list(r)) for r in g]


def fn_rows():
    r = []
    lv = lambda shapes: ([h for h, _ in shapes], [w for _, w in shapes], len(shapes))      # noqa: E731
    conv = [([(h, w)], ci, co) for h, w, ci, co in VGG] + [(FPN, 256, 256), ([(1, 1)], 64, 64), ([(1, 1)] * 8, 64, 64), ([(20, 22)], 64, 64),
            ([(2, 600)], 64, 64), ([(3, 515)], 64, 128), ([(40, 40)], 64, 192), ([(40, 40)], 192, 64), ([(21, 24)], 128, 256), ([(64, 64)], 32, 512),
            ([(9, 14)], 128, 128), ([(5, 5)], 0, 64), ([(5, 5)], 64, 63), ([(0, 5)], 64, 64), ([(5, 5)] * 9, 64, 64)]
    for shapes, ci, co in conv:
        H, W, n = lv(shapes)
        r.append(("frcnn_conv3x3_f32_workspace", [H, W, n, ci, co]))
        r.append(("frcnn_conv3x3_f32_u_floats", [H, W, n, ci, co]))
        r.append(("frcnn_conv3x3_f32_xt_floats", [H, W, n, ci]))
        r.append(("frcnn_conv3x3_f32_xt_floats", [H, W, n, co]))
        r.append(("frcnn_conv3x3_f32_relu_bits_words", [H, W, n, co]))
    for shapes, c in [(FPN, 256), ([(37, 62)], 512), ([(9, 14)], 128), ([(1, 1)], 128), (FPN, 64), (FPN, 0), ([(1, 1)] * 9, 128)]:
        H, W, n = lv(shapes)
        r.append(("frcnn_rpn_conv3x3_f32_workspace", [H, W, n, c]))
    r.append(("frcnn_gemm_nt_f32_workspace", []))
    for h, co in [(600, 64), (1, 4), (800, 64), (0, 64), (600, 0)]:
        r.append(("frcnn_conv3x3_c3_wgrad_workspace", [h, co]))
    for shapes, c, n_rois in [(FPN[:4], 256, 512), (FPN[:4], 256, 1000), (FPN[:4], 256, 0), ([(1, 1)], 1, 1), ([(37, 62)], 512, 128), ([(8, 16)], 32, 1),
                              ([(9, 17)], 33, 15), (FPN[:4], 0, 10), (FPN[:4], 256, -1), ([(5, 5)] * 9, 8, 10)]:
        H, W, n = lv(shapes)
        r.append(("frcnn_ms_roi_align_bwd_workspace", [H, W, n, c, n_rois]))
    for src, size, max_size in [([375, 500, 333, 500, 500, 375, 480, 640], 600, 1000), ([1, 1, 1, 1, 1, 1, 1, 1], 1, 1),
                                ([375, 500, 333, 500, 500, 375, 480, 640], 320, 512), ([375, 500, 0, 500, 500, 375, 480, 640], 600, 1000),
                                ([375, 500, 333, 500, 500, 375, 480, 640], 16384, 32767), ([32767, 32767] * 4, 2, 2)]:
        r.append(("frcnn_mosaic_workspace", [src, size, max_size]))
    for h, w in [(375, 500), (1, 1), (32767, 32767), (0, 5), (5, 32768)]:
        r.append(("frcnn_photometric_workspace", [h, w]))
    for a in [(375, 500, 750, 1000), (1, 1, 1, 1), (375, 500, 1500, 2000), (375, 500, 374, 500), (0, 1, 1, 1), (1, 1, 32768, 1)]:
        r.append(("frcnn_zoom_out_workspace", list(a)))
    for a in [(375, 500, 600, 800, 512, 512), (480, 640, 800, 1067, 384, 600), (1, 1, 1, 1, 1, 1), (1333, 2000, 600, 900, 1, 1),
              (375, 500, 600, 800, 600, 800), (375, 500, 600, 800, 601, 800), (375, 500, 600, 800, 0, 8), (0, 500, 600, 800, 8, 8)]:
        r.append(("frcnn_resize_crop_workspace", list(a)))
    for n in [1, 2, 3, 1000, 0, -1]:
        r.append(("frcnn_grad_norm_workspace_bytes", [n]))
    for t, n in [(1, 1), (40, 1000), (3, 2), (0, 1), (1, 0), (-1, 5)]:
        r.append(("frcnn_tensor_stats_workspace_bytes", [t, n]))
    return r


def bind(lib):
    for name, sig in SIG.items():
        f = getattr(lib, name)
        f.restype = C.c_size_t
        f.argtypes = [{"i": C.c_int, "q": C.c_int64, "I": C.c_void_p}[c] for c in sig]


def call(lib, name, args):
    keep = [(C.c_int32 * len(a))(*a) if isinstance(a, list) else a for a in args]
    return int(getattr(lib, name)(*[C.cast(a, C.c_void_p) if isinstance(a, C.Array) else a for a in keep]))


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
    lib = C.CDLL(so)
    bind(lib)
    rows = [[name, args, call(lib, name, args)] for name, args in op_rows() + fn_rows()]
    with open(out, "w") as f:
        f.write('{"cu_count": 256,\n "sig": %s,\n "rows": [\n' % json.dumps(SIG))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print("%d rows from %s -> %s" % (len(rows), so, out))


if __name__ == "__main__":
    main()
