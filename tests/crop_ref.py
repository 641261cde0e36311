"""The crop of the wired pipeline restated for the tests (new_datasets/transforms.py:16-56 behind resize, :76-132; CenterCrop :183-192).

Image side: oracle.preprocess_image (bit-identical to Pillow's 8-bit bilinear resize, tests/test_preprocess.py) and numpy slicing; an
equal size is a copy, as Pillow makes one.  Box side: the reference's torch expressions on CPU float32 tensors.  Pinned to the
reference's own code by tests/golden/crop.npz (tests/test_crop_host.py); the GPU tests compare the kernels with it and with the file."""
import os

import numpy as np
import torch

from oracle import oracle as orc


def load_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crop.npz"), allow_pickle=False)


def case_names(gold):
    return [str(s) for s in gold["case_names"]]


def case_inputs(gold, name):
    """(img, boxes, labels, iscrowd or None, resize_hw, region) of a stored case."""
    meta = gold[name + "_meta"]                                           # H1, W1, i, j, ch, cw, has_iscrowd, has_area
    return (gold[name + "_img"], gold[name + "_boxes"], gold[name + "_labels"], gold[name + "_iscrowd"] if int(meta[6]) else None,
            (int(meta[0]), int(meta[1])), tuple(int(v) for v in meta[2:6]))


def resize_u8(img, out_hw):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if tuple(img.shape[:2]) == (int(out_hw[0]), int(out_hw[1])):
        return img.copy()
    return orc.preprocess_image(img, (int(out_hw[0]), int(out_hw[1])))[0]


def resize_boxes(boxes, new_hw, old_hw):
    """transforms.py:111-117: the ratios are Python floats, as_tensor rounds them to float32, the product is float32."""
    rh, rw = float(new_hw[0]) / float(old_hw[0]), float(new_hw[1]) / float(old_hw[1])
    return boxes * torch.as_tensor([rw, rh, rw, rh])


def crop_boxes(boxes, region):
    """transforms.py:29-35, 48-49 -> (clipped boxes, area, keep)."""
    i, j, h, w = (int(v) for v in region)
    max_size = torch.as_tensor([w, h], dtype=torch.float32)
    c = boxes - torch.as_tensor([j, i, j, i])
    c = torch.min(c.reshape(-1, 2, 2), max_size)
    c = c.clamp(min=0)
    area = (c[:, 1, :] - c[:, 0, :]).prod(dim=1)
    keep = torch.all(c[:, 1, :] > c[:, 0, :], dim=1)
    return c.reshape(-1, 4), area, keep


def crop_ref(img, boxes, labels, iscrowd, resize_hw, region, live=None):
    """uint8 HWC array, [n, 4] float32, [n] int64, [n] int64 or None, (H1, W1) or None, (i, j, ch, cw) ->
    (image uint8 [ch, cw, 3], boxes [m, 4], labels [m], area [m], iscrowd [m] or None).  live: only the first `live` rows count."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    H1, W1 = (h, w) if resize_hw is None else (int(resize_hw[0]), int(resize_hw[1]))
    i, j, ch, cw = (int(v) for v in region)
    assert 0 <= i and 0 <= j and 1 <= ch <= H1 - i and 1 <= cw <= W1 - j, "the region must lie inside the resized frame"
    n = len(boxes) if live is None else max(0, min(int(live), len(boxes)))
    out = resize_u8(img, (H1, W1))[i:i + ch, j:j + cw].copy()
    b = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)[:n].copy())
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)[:n].copy())
    c, area, keep = crop_boxes(resize_boxes(b, (H1, W1), (h, w)), region)
    crowd = None if iscrowd is None else torch.from_numpy(np.ascontiguousarray(iscrowd, dtype=np.int64).reshape(-1)[:n].copy())[keep].numpy()
    return out, c[keep].numpy(), lab[keep].numpy(), area[keep].numpy(), crowd


def center_crop_region(h, w, size):
    """transforms.py:187-192."""
    crop_height, crop_width = size
    return int(round((h - crop_height) / 2.)), int(round((w - crop_width) / 2.)), int(crop_height), int(crop_width)


def seeded_case(seed, h, w, resize_hw, region, n, iscrowd=True):
    """A frame and n boxes around a region of its resized frame: about a third inside, a third cut, a third outside."""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    H1, W1 = resize_hw or (h, w)
    i, j, ch, cw = region
    x1, y1 = rng.uniform(j - cw, j + cw, n), rng.uniform(i - ch, i + ch, n)
    b = np.stack([x1, y1, x1 + rng.uniform(1, cw, n), y1 + rng.uniform(1, ch, n)], 1) * np.array([w / W1, h / H1, w / W1, h / H1])
    return img, b.astype(np.float32), rng.randint(0, 90, n).astype(np.int64), rng.randint(0, 2, n).astype(np.int64) if iscrowd else None


def full_frame():
    """The 480 x 640 frame of the golden file's full-size case, from its seed: (img, boxes, labels, iscrowd)."""
    rng = np.random.RandomState(480640)
    img = rng.randint(0, 256, (480, 640, 3)).astype(np.uint8)
    x1, y1 = rng.uniform(0, 640 * 0.8, 24), rng.uniform(0, 480 * 0.8, 24)
    boxes = np.stack([x1, y1, x1 + rng.uniform(10, 200, 24), y1 + rng.uniform(10, 200, 24)], 1).astype(np.float32)
    return img, boxes, rng.randint(0, 90, 24).astype(np.int64), rng.randint(0, 2, 24).astype(np.int64)


def final_stage_ref(img, boxes, flip, size, max_size, size_divisible=32, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """hflip, resize(size, max_size), ToTensor, Normalize and the zero pad on the frame -> (x [3, PH, PW], normalised boxes, (oh, ow))."""
    from faster_rcnn_pytorch_amd.transforms import get_size, padded_size
    h, w = img.shape[:2]
    oh, ow = get_size((w, h), size, max_size)
    pad = padded_size(oh, ow, size_divisible) if size_divisible else None
    x = orc.preprocess_image(img, (oh, ow), pad, flip, mean, std)[1]
    return x, orc.preprocess_boxes(boxes, (w, h), (ow, oh), flip), (oh, ow)
