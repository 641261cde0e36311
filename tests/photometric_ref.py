"""photometric_distort_ and zoom_out_ (datasets/transforms_.py:38-58,130-147) restated in numpy for the tests.

Every form below is the arithmetic Pillow 12.2 performs for the calls torchvision's PIL backend makes (ImageEnhance.Brightness /
Contrast / Color -> Image.blend; convert("HSV"), a uint8 shift of the H plane, convert("RGB"); ImageStat's median), operation for
operation and in the same number formats.  Pinned to the reference's own code under Pillow by tests/golden/photometric.npz
(tests/test_photometric_host.py) and, where Pillow is importable, to Pillow directly; the GPU tests compare the kernels of
csrc/photometric.hip with it and with the golden file.  Test infrastructure only."""
import os

import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
F32, F64 = np.float32, np.float64


def load_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric.npz"), allow_pickle=False)


def seeded_frame(seed, h, w):
    """The frames the golden file stores as a seed only."""
    return np.random.RandomState(int(seed)).randint(0, 256, (int(h), int(w), 3)).astype(np.uint8)


def cube():
    """4096 x 4096: every colour once, R the slowest."""
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.ascontiguousarray(np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3))


def case_input(gold, name):
    """The input frame of a photometric case of the golden file (stored whole, or regenerated from its seed)."""
    if name + "_img" in gold.files:
        return gold[name + "_img"]
    return gold["p_order_img"] if name.startswith("p_order") else seeded_frame(*gold[name + "_seed"])


def hue_shift(factor):
    """uint8(int32(f * 255)): the product in float64, truncated toward zero, mod 256."""
    return int(float(factor) * 255.0) & 0xFF


def luma(img):
    """convert("L"): (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    p = img.astype(np.int64)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate, image, alpha):
    """Image.blend(degenerate, image, alpha) per byte: alpha in binary32, t = a + alpha * (b - a) with a rounding after each operation."""
    al = F32(alpha)
    a, b = degenerate.astype(F32), image.astype(F32)
    t = a + (al * (b - a)).astype(F32)
    if 0.0 <= al <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def contrast_mean(img):
    """int(sum(L) / count + 0.5) in float64: the degenerate of ImageEnhance.Contrast."""
    L = luma(img)
    return int(float(int(L.astype(np.int64).sum())) / L.size + 0.5)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def saturation(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, -1), img, f)


def _clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def rgb_to_hsv(img):
    r, g, b = (img[..., k].astype(np.int32) for k in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = mx == mn
    cr = np.where(grey, 1, mx - mn).astype(F32)
    s = cr / np.where(grey, 1, mx).astype(F32)
    rc, gc, bc = ((mx - c).astype(F32) / cr for c in (r, g, b))
    h_r = bc - gc
    h_g = (2.0 + rc.astype(F64) - bc.astype(F64)).astype(F32)
    h_b = (4.0 + gc.astype(F64) - rc.astype(F64)).astype(F32)
    h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b))
    h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
    H = _clip8((h.astype(F64) * 255.0).astype(np.int64))
    S = _clip8((s.astype(F64) * 255.0).astype(np.int64))
    return np.stack([np.where(grey, 0, H), np.where(grey, 0, S), mx], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    H, S, V = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    x = H.astype(F64) * 6.0 / 255.0
    i = np.floor(x)
    f = (x - i).astype(F32).astype(F64)
    fs = (S.astype(F64) / 255.0).astype(F32).astype(F64)
    v = V.astype(F64)
    p = _clip8(_c_round(v * (1.0 - fs)))
    q = _clip8(_c_round(v * (1.0 - fs * f)))
    t = _clip8(_c_round(v * (1.0 - fs * (1.0 - f))))
    k = i.astype(np.int64) % 6
    table = ((V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q))
    out = np.empty(hsv.shape, np.uint8)
    for c in range(3):
        out[..., c] = np.select([k == j for j in range(6)], [table[j][c] for j in range(6)])
    grey = S == 0
    out[grey] = V[grey][:, None]
    return out


def _c_round(x):
    """C round(): halves away from zero (the values here are never negative)."""
    r = np.floor(x)
    return np.where(x - r >= 0.5, r + 1.0, r)


def hue(img, shift):
    """adjust_hue with the shift already formed (hue_shift): a shift of 0 still goes through both conversions."""
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)).astype(np.uint8)
    return hsv_to_rgb(hsv)


OPS = (brightness, contrast, saturation, hue)


def plan(order, factors):
    """The device plan int32[8] (include/frcnn_hip.h): four (op, param) slots; param = the binary32 bits of alpha, or the hue shift."""
    out = np.full(8, -1, np.int32)
    for k, op in enumerate(order):
        out[2 * k] = op
        out[2 * k + 1] = hue_shift(factors[op]) if op == HUE else int(np.array(factors[op], F32).view(np.int32))
    return out


def apply_plan(img, pl):
    """A plan as the kernels read it: ops outside 0..3 are skipped, and so is an op from its second appearance on."""
    pl = np.asarray(pl, np.int32).reshape(4, 2)
    out, seen = np.ascontiguousarray(img, dtype=np.uint8), set()
    for op, param in pl:
        op = int(op)
        if op < 0 or op > 3 or op in seen:
            continue
        seen.add(op)
        out = hue(out, int(param) & 0xFF) if op == HUE else OPS[op](out, float(np.array(param, np.int32).view(F32)))
    return out


def photometric(img, order, factors):
    """photometric_distort_ with its draws given: order = the shuffled op ids, factors[op] = the factor drawn for op."""
    return apply_plan(img, plan(order, factors))


def median(img):
    """ImageStat's median per channel: the first level whose cumulative count exceeds count // 2."""
    flat = img.reshape(-1, 3)
    out = []
    for c in range(3):
        cum = np.cumsum(np.bincount(flat[:, c], minlength=256))
        out.append(int(np.argmax(cum > flat.shape[0] // 2)))
    return tuple(out)


def zoom_out(img, boxes, new_hw, top_left):
    """zoom_out_ with its draws given -> (canvas uint8 [new_h, new_w, 3], boxes float32 [n, 4])."""
    h, w = img.shape[:2]
    (new_h, new_w), (top, left) = new_hw, top_left
    canvas = np.empty((new_h, new_w, 3), np.uint8)
    canvas[:] = np.array(median(img), np.uint8)
    canvas[top:top + h, left:left + w] = img
    b = np.asarray(boxes, F32).reshape(-1, 4)
    return canvas, b + np.array([left, top, left, top], F32)
