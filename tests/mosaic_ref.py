"""The mosaic protocol restated for the tests (datasets/mosaic_transform.py:39-95 on datasets/transforms_.py:61-127,150-178).

Image side: oracle.preprocess_image (bit-identical to Pillow's 8-bit bilinear resize, tests/test_preprocess.py), numpy slicing and
pasting.  Box side: the reference's torch expressions on CPU float32 tensors.  Pinned to the reference's own code by
tests/golden/mosaic.npz (tests/test_mosaic_host.py); the GPU tests compare the kernels with it and with the golden file."""
import os

import numpy as np
import torch

from oracle import oracle as orc

SMALL = ("small_capped", "small_down", "small_mixed")          # the small cases of tests/golden/mosaic.npz


def load_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mosaic.npz"), allow_pickle=False)


def small_inputs(gold, name):
    """(imgs, boxes, labels, regions, size, max_size) of a small case: the arguments of mosaic_ref."""
    size, max_size = (int(v) for v in gold[name + "_meta"])
    return ([gold["%s_img%d" % (name, k)] for k in range(4)], [gold["%s_boxes%d" % (name, k)] for k in range(4)],
            [gold["%s_labels%d" % (name, k)] for k in range(4)], gold[name + "_regions"], size, max_size)


def full_inputs(gold):
    """The size-600 case: the frames load_mosaic drew, regenerated from their seeds, and the regions it recorded."""
    frames = [full_frame(int(i)) for i in gold["full_order"]]
    return [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], gold["full_regions"], 600, 1333


def first_resize_hw(h, w, size, max_size=1333):
    """resize_'s size logic for a scalar size, in its own order of float operations (transforms_.py:93-114) -> (H1, W1)."""
    if max_size is not None:
        lo, hi = float(min(h, w)), float(max(h, w))
        if size / lo * hi > max_size:
            size = int(round(max_size / hi * lo))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def resize_u8(img, out_hw):
    return orc.preprocess_image(img, (int(out_hw[0]), int(out_hw[1])))[0]


def scale_boxes(boxes, new_hw, old_hw):
    """transforms_.py:118-125: the ratios are Python floats, the product is float32."""
    rh, rw = float(new_hw[0]) / float(old_hw[0]), float(new_hw[1]) / float(old_hw[1])
    return boxes * torch.as_tensor([rw, rh, rw, rh]).unsqueeze(0)


def crop_keep(boxes, region):
    """transforms_.py:152-168 -> (clipped boxes, keep mask)."""
    i, j, h, w = (int(v) for v in region)
    c = boxes - torch.as_tensor([j, i, j, i])
    c = torch.min(c.reshape(-1, 2, 2), torch.as_tensor([w, h], dtype=torch.float32)).clamp(min=0)
    keep = torch.all(c[:, 1, :] > c[:, 0, :], dim=1)
    c = c.reshape(-1, 4)
    d, dc = boxes[:, 2:] - boxes[:, :2], c[:, 2:] - c[:, :2]
    keep = keep * ((dc[:, 0] * dc[:, 1]) / (d[:, 0] * d[:, 1]) > 0.3)
    return c, keep


def mosaic_ref(imgs, boxes, labels, regions, size, max_size=1333):
    """Four uint8 HWC arrays, four [n, 4] float32 box arrays, four [n] int64 label arrays, regions [4][4] (i, j, h, w) ->
    (canvas uint8 [2 size, 2 size, 3], boxes float32 [M, 4], labels int64 [M], fallback uint8 [4], used regions int32 [4, 4])."""
    canvas = np.zeros((2 * size, 2 * size, 3), np.uint8)
    out_b, out_l, fallback, used = [], [], np.zeros(4, np.uint8), np.zeros((4, 4), np.int32)
    for k in range(4):
        img = np.ascontiguousarray(imgs[k], dtype=np.uint8)
        h, w = img.shape[:2]
        H1, W1 = first_resize_hw(h, w, size, max_size)
        img1 = resize_u8(img, (H1, W1))                                   # a real uint8 image between the two resizes
        b = torch.from_numpy(np.ascontiguousarray(boxes[k], dtype=np.float32).reshape(-1, 4))
        lab = torch.from_numpy(np.ascontiguousarray(labels[k], dtype=np.int64).reshape(-1))
        b1 = scale_boxes(b, (H1, W1), (h, w))
        c, keep = crop_keep(b1, regions[k])
        if int(keep.sum()) == 0:                                          # transforms_.py:174-176
            fallback[k], reg, bk, lk = 1, (0, 0, H1, W1), b1, lab
        else:
            reg, bk, lk = tuple(int(v) for v in regions[k]), c[keep], lab[keep]
        i, j, rh, rw = reg
        used[k] = reg
        tile = resize_u8(img1[i:i + rh, j:j + rw], (size, size))
        bk = scale_boxes(bk, (size, size), (rh, rw))
        sx, sy = (k & 1) * size, (k >> 1) * size
        bk = bk.clone()
        bk[:, 0] = bk[:, 0] + sx                                         # mosaic_transform.py:7-12
        bk[:, 1] = bk[:, 1] + sy
        bk[:, 2] = bk[:, 2] + sx
        bk[:, 3] = bk[:, 3] + sy
        canvas[sy:sy + size, sx:sx + size] = tile
        out_b.append(bk)
        out_l.append(lk)
    return canvas, torch.cat(out_b).numpy(), torch.cat(out_l).numpy(), fallback, used


FULL_SHAPES = ((375, 500), (500, 375), (333, 500), (375, 500), (480, 640), (400, 400))          # the full-size case's six-frame "dataset"; seeds 100 + index


def full_frame(index):
    rng = np.random.RandomState(100 + index)
    h, w = FULL_SHAPES[index]
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    x1, y1 = rng.uniform(0, w * 0.6, 8), rng.uniform(0, h * 0.6, 8)
    boxes = np.stack([x1, y1, x1 + rng.uniform(20, w * 0.4, 8), y1 + rng.uniform(20, h * 0.4, 8)], 1).astype(np.float32)
    return img, boxes, rng.randint(0, 20, 8).astype(np.int64)


def final_stage_ref(canvas, boxes, flip=False, out_size=800, out_max_size=1333, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """The ordinary transform on the canvas (datasets/build.py:15-19): flip, RandomResize([out_size]), ToTensor, Normalize; no pad."""
    from faster_rcnn_pytorch_amd.transforms import get_size
    h, w = canvas.shape[:2]
    oh, ow = get_size((w, h), out_size, out_max_size)
    x = orc.preprocess_image(canvas, (oh, ow), None, flip, mean, std)[1]
    return x, orc.preprocess_boxes(boxes, (w, h), (ow, oh), flip), (oh, ow)
