"""Device-side input stage: the reference's per-sample transforms and pad-to-32 collate for ONE frame
that is already in HBM as uint8 HWC, on the kernels of csrc/preprocess.hip.

Mirrors (file:line under the reference):
  new_datasets/transforms.py:57-72    hflip (image + boxes)
  new_datasets/transforms.py:76-132   resize(image, target, size, max_size) incl. get_size_with_aspect_ratio
  new_datasets/transforms.py:238-281  ToTensor, Normalize (boxes / (w, h))
  new_datasets/build.py:20-33, datasets/build.py:10-24   Compose([RandomHorizontalFlip, Resize(800, 1333), ToTensor, Normalize])
  new_datasets/coco_dataset.py:49-66  batched_tensor_from_tensor_list (zero pad to a multiple of 32)
JPEG decoding and the dataset classes stay out of scope; the flip coin is the caller's (random.random() < p).

Mosaic augmentation (config.py:16 --mosaic_transform), on the kernels of csrc/mosaic.hip:
  datasets/voc_dataset.py:145-156, datasets/coco_dataset.py:154-157   where the option is applied (the 0.5 coin is the caller's)
  datasets/mosaic_transform.py:39-95   load_mosaic: three more frames (the caller's choice), the per-tile Compose, shift, concat
  datasets/mosaic_transform.py:7-26    shift_mosaic_boxes, get_concat_h_cut_center, get_concat_v_cut_center
  datasets/transforms_.py:61-127       resize_ (both resizes of a tile; its own order of float operations in the size logic)
  datasets/transforms_.py:150-178      crop_ incl. the hand-back of the uncropped frame when no box survives
  datasets/transforms_.py:278-288      RandomSizeCrop (DeviceMosaicStage.draw_regions: the same distribution, not the same stream)
  datasets/build.py:15-19              the ordinary transform the canvas then enters (DeviceMosaicStage.__call__)

Photometric distortion and zoom-out (the richer recipe of datasets/build.py:28-42), on the kernels of csrc/photometric.hip:
  datasets/transforms_.py:38-58, 240-247   photometric_distort_, RandomPhotoDistortion (draw_photometric, photometric_plan, photometric_distort)
  datasets/transforms_.py:130-147, 291-299 zoom_out_, RandomZoomOut (draw_zoom_out, zoom_out)
  DeviceAugmentStage: photometric, zoom-out, then the DeviceInputStage.  The coins (random.random() < p) stay with the caller.
transforms_.py's RandomSizeCrop alone (:278-288) has no device form: crop_ hands back the uncropped frame when no box survives, so the
output SHAPE would depend on data in device memory and reading it would be a host synchronisation (docs/PARITY.md).

Crop and the multi-scale crop recipe (sketched in datasets/build.py:27-39) of the WIRED pipeline, on the kernels of csrc/crop.hip:
  new_datasets/transforms.py:16-56     crop: always crops, drops boxes that lose a side (crop; a device count behind fixed-capacity lists)
  new_datasets/transforms.py:162-192   RandomCrop, RandomSizeCrop, CenterCrop (draw_random_crop, draw_random_size_crop, center_crop_region)
  new_datasets/transforms.py:205-239   RandomResize, RandomSelect (DeviceMultiScaleStage.draw)
Not built: pad / RandomPad (:135-145, 216-223; no recipe uses them) and everything about masks.
"""
import collections
import ctypes as C
import math
import random

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .ops import _ptr, _req, _stream, _workspace, _np_ptr

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def get_size_with_aspect_ratio(image_size, size, max_size=None):
    """transforms.py:79-99.  image_size = (w, h) as PIL reports it; returns (oh, ow)."""
    w, h = int(image_size[0]), int(image_size[1])
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def get_size(image_size, size, max_size=None):
    """transforms.py:101-105: a (w, h) tuple is taken as is (reversed), a scalar is the shorter side."""
    if isinstance(size, (list, tuple)):
        return tuple(size[::-1])
    return get_size_with_aspect_ratio(image_size, size, max_size)


def padded_size(h, w, size_divisible=32):
    """coco_dataset.py:57-60."""
    stride = float(size_divisible)
    return int(math.ceil(float(h) / stride) * stride), int(math.ceil(float(w) / stride) * stride)


def preprocess_image(img, out_hw, pad_hw=None, flip=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, want_u8=False):
    """uint8 HWC [h, w, 3] on a HIP device -> float32 [3, pad_h, pad_w] (and optionally the resized uint8 [oh, ow, 3])."""
    img = _frame(img)
    h, w = int(img.shape[0]), int(img.shape[1])
    oh, ow = int(out_hw[0]), int(out_hw[1])
    ph, pw = (oh, ow) if pad_hw is None else (int(pad_hw[0]), int(pad_hw[1]))
    dev = img.device
    out = torch.empty((3, ph, pw), dtype=torch.float32, device=dev)
    u8 = torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    m = np.ascontiguousarray(mean, dtype=np.float32)
    s = np.ascontiguousarray(std, dtype=np.float32)
    nb = _lib.workspace_bytes(_lib.OP_PREPROCESS, (h << 32) | w, (oh << 32) | ow)
    ws = _workspace(dev, nb)
    with torch.cuda.device(dev):
        check(lib.frcnn_preprocess_image(_ptr(img), h, w, int(bool(flip)), oh, ow, ph, pw, _np_ptr(m), _np_ptr(s), _ptr(out), _ptr(u8),
                                         _ptr(ws), nb, _stream()), "preprocess_image")
    return (out, u8) if want_u8 else out


def preprocess_boxes(boxes, src_wh, out_wh, flip=False):
    """xyxy boxes in source pixels -> the normalised boxes the model takes (hflip, resize ratios, / resized (w, h))."""
    boxes = _req(boxes, torch.float32, "boxes").reshape(-1, 4)
    out = torch.empty_like(boxes)
    with torch.cuda.device(boxes.device):
        check(lib.frcnn_preprocess_boxes(_ptr(boxes), boxes.shape[0], int(src_wh[0]), int(src_wh[1]), int(bool(flip)), int(out_wh[0]),
                                         int(out_wh[1]), _ptr(out), _stream()), "preprocess_boxes")
    return out


class DeviceInputStage:
    """Compose([RandomHorizontalFlip, Resize(size, max_size), ToTensor, Normalize]) + the batch-1 collate, on the device.

    stage(img_u8_hwc, boxes_xyxy_pixels=None, flip=False) -> (x [1, 3, PH, PW] float32, boxes normalised or None,
    {'size': (oh, ow), 'padded': (PH, PW), 'orig_size': (h, w)}).  size_divisible=None skips the pad (the VOC loader)."""

    def __init__(self, size=800, max_size=1333, mean=IMAGENET_MEAN, std=IMAGENET_STD, size_divisible=32):
        self.size, self.max_size, self.mean, self.std, self.size_divisible = size, max_size, tuple(mean), tuple(std), size_divisible

    def __call__(self, img, boxes=None, flip=False):
        h, w = int(img.shape[0]), int(img.shape[1])
        oh, ow = get_size((w, h), self.size, self.max_size)
        ph, pw = padded_size(oh, ow, self.size_divisible) if self.size_divisible else (oh, ow)
        x = preprocess_image(img, (oh, ow), (ph, pw), flip, self.mean, self.std)
        b = preprocess_boxes(boxes, (w, h), (ow, oh), flip) if boxes is not None else None
        return x[None], b, {"size": (oh, ow), "padded": (ph, pw), "orig_size": (h, w)}


# ---------------------------------------------------------------------------------------------------------------------------
# mosaic augmentation
# ---------------------------------------------------------------------------------------------------------------------------
def mosaic_resize_hw(h, w, size, max_size=1333):
    """The first resize of a mosaic tile: resize_'s size logic for a scalar size, in ITS order of float operations
    (transforms_.py:93-114; get_size_with_aspect_ratio above mirrors the other transforms file) -> (H1, W1)."""
    h, w = int(h), int(w)
    if max_size is not None:
        lo, hi = float(min(h, w)), float(max(h, w))
        if size / lo * hi > max_size:
            size = int(round(max_size / hi * lo))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


class MosaicResult(collections.namedtuple("MosaicResult", "canvas_u8 boxes labels count fallback")):
    """canvas_u8 uint8 [2 size, 2 size, 3]; boxes float32 [N, 4] and labels int64 [N] with the first `count` rows live (tile order,
    each tile's own order) and zeros behind them; count int32 [1] and fallback uint8 [4] (1: the tile was not cropped) on the device."""
    __slots__ = ()

    def to_host(self):
        """What load_mosaic returns: (uint8 array, boxes[:count], labels[:count]).  Synchronises."""
        n = int(self.count.item())
        return self.canvas_u8.cpu().numpy(), self.boxes[:n].cpu().numpy(), self.labels[:n].cpu().numpy()


def mosaic(imgs, boxes, labels, regions, size, max_size=1333, counts=None):
    """load_mosaic (mosaic_transform.py:39-95) for four frames already on the device, without a host read-back.

    imgs: four uint8 HWC tensors.  boxes / labels: four float32 [n_k, 4] / int64 [n_k] tensors (pixel xyxy of their frame), or one
    tile-major tensor each plus counts = (n_0, n_1, n_2, n_3).  regions: [4][4] host integers, (i, j, h, w) of each tile's crop in its
    RESIZED frame (DeviceMosaicStage.draw_regions).  Whether a tile is cropped is decided on the device (crop_ hands back the uncropped
    frame when no box survives); the result has fixed shapes and a device count, so the call can be captured into a graph."""
    if len(imgs) != 4:
        raise ValueError("mosaic takes four frames, got %d" % len(imgs))
    imgs = [_frame(im, "imgs[%d]" % k) for k, im in enumerate(imgs)]
    dev = imgs[0].device
    if counts is None:
        if len(boxes) != 4 or len(labels) != 4:
            raise ValueError("mosaic takes four box and four label tensors (or one of each plus counts)")
        counts = [int(b.shape[0]) for b in boxes]
        if [int(l.shape[0]) for l in labels] != counts:
            raise ValueError("boxes and labels disagree about the number of rows per tile")
        boxes = torch.cat([_req(b, torch.float32, "boxes").reshape(-1, 4) for b in boxes])
        labels = torch.cat([_req(l, torch.int64, "labels").reshape(-1) for l in labels])
    boxes = _req(boxes, torch.float32, "boxes").reshape(-1, 4)
    labels = _req(labels, torch.int64, "labels").reshape(-1)
    counts = [int(c) for c in counts]
    n = sum(counts)
    if len(counts) != 4 or min(counts) < 0 or boxes.shape[0] != n or labels.shape[0] != n:
        raise ValueError("counts %s do not describe %d boxes and %d labels" % (counts, boxes.shape[0], labels.shape[0]))
    size = int(size)
    src_hw = np.array([[im.shape[0], im.shape[1]] for im in imgs], np.int32)
    reg = np.ascontiguousarray(regions, dtype=np.int32).reshape(4, 4)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ms = 0 if max_size is None else int(max_size)
    canvas = torch.empty((2 * size, 2 * size, 3), dtype=torch.uint8, device=dev)
    boxes_out, labels_out = torch.empty_like(boxes), torch.empty_like(labels)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    fallback = torch.empty(4, dtype=torch.uint8, device=dev)
    nb = int(lib.frcnn_mosaic_workspace(_np_ptr(src_hw), size, ms))
    if nb == 0:
        raise ValueError("mosaic: unsupported shapes %s at size %d (sides of 1 .. 32767 before and after the first resize, 2 * size < 32768)"
                         % (src_hw.tolist(), size))
    ws = _workspace(dev, nb)
    srcs = (C.c_void_p * 4)(*[im.data_ptr() for im in imgs])
    with torch.cuda.device(dev):
        check(lib.frcnn_mosaic(srcs, _np_ptr(src_hw), size, ms, _np_ptr(reg), _ptr(boxes), _ptr(labels), _np_ptr(offs), _ptr(canvas),
                               _ptr(boxes_out), _ptr(labels_out), _ptr(count), _ptr(fallback), _ptr(ws), nb, _stream()), "mosaic")
    return MosaicResult(canvas, boxes_out, labels_out, count, fallback)


class DeviceMosaicStage:
    """load_mosaic followed by the ordinary transform (datasets/build.py:15-19: flip, RandomResize([out_size], out_max_size), ToTensor,
    Normalize), on the device.  The random draws stay with the caller: which three other frames, the dataset's `random.random() > 0.5`
    (voc_dataset.py:145), the flip coin, and the crop regions -- draw_regions() draws those with the reference's distribution.

    stage(imgs, boxes, labels, regions, flip=False) -> (x [1, 3, PH, PW] float32, normalised boxes [N, 4], labels [N], count int32 [1]
    on the device, meta).  The final stage is applied to all N rows (it is elementwise): rows at and above count are padding."""

    def __init__(self, size=600, max_size=1333, min_crop=384, out_size=800, out_max_size=1333, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 size_divisible=None):
        self.size, self.max_size, self.min_crop = int(size), max_size, int(min_crop)        # the reference fixes max_size = 1333, min_crop = 384
        self.final = DeviceInputStage(out_size, out_max_size, mean, std, size_divisible)

    def draw_regions(self, shapes, rng=random):
        """RandomSizeCrop(min_crop, size) (transforms_.py:284-286) for four source shapes (h, w): w in [min_crop, min(W1, size)], h in
        [min_crop, min(H1, size)], the corner uniform over the positions that fit.  The reference's DISTRIBUTION, not its random stream
        (torchvision's get_params draws the corner from torch's generator).  rng: anything with randint(a, b), both ends included."""
        out = []
        for h, w in shapes:
            H1, W1 = mosaic_resize_hw(h, w, self.size, self.max_size)
            if min(H1, W1, self.size) < self.min_crop:
                raise ValueError("a %d x %d frame resizes to %d x %d: smaller than min_crop %d" % (h, w, H1, W1, self.min_crop))
            cw = rng.randint(self.min_crop, min(W1, self.size))
            ch = rng.randint(self.min_crop, min(H1, self.size))
            out.append((rng.randint(0, H1 - ch), rng.randint(0, W1 - cw), ch, cw))
        return out

    def __call__(self, imgs, boxes, labels, regions, flip=False, counts=None):
        r = mosaic(imgs, boxes, labels, regions, self.size, self.max_size, counts)
        x, b, meta = self.final(r.canvas_u8, r.boxes, flip)
        meta["fallback"] = r.fallback
        return x, b, r.labels, r.count, meta


# ---------------------------------------------------------------------------------------------------------------------------
# photometric distortion and zoom-out
# ---------------------------------------------------------------------------------------------------------------------------
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def photometric_plan(order, factors):
    """The host side of photometric_distort_ (transforms_.py:50-57): order = the op ids in the order drawn (each of BRIGHTNESS, CONTRAST,
    SATURATION, HUE at most once; fewer than four is allowed), factors = {op: factor} or a sequence indexed by op -> the int32[8] plan
    frcnn_photometric reads: four (op, param) slots, -1 for an unused slot.  param: the factor rounded to binary32, as bits (Image.blend
    takes a C float); for HUE the shift uint8(int32(factor * 255)): the product in binary64, truncated toward zero, mod 256."""
    order = [int(op) for op in order]
    if len(order) > 4 or len(set(order)) != len(order) or any(op < 0 or op > 3 for op in order):
        raise ValueError("photometric_plan: order %s must name each of the ops 0..3 at most once" % (order,))
    plan = np.full(8, -1, np.int32)
    for k, op in enumerate(order):
        f = float(factors[op])
        if not math.isfinite(f):
            raise ValueError("photometric_plan: factor %r of op %d is not finite" % (f, op))
        plan[2 * k] = op
        plan[2 * k + 1] = (int(f * 255.0) & 0xFF) if op == HUE else int(np.array(f, np.float32).view(np.int32))
    return plan


def draw_photometric(rng=random):
    """photometric_distort_'s draws (transforms_.py:50-56): a shuffled order, uniform(0.5, 1.5) for brightness / contrast / saturation and
    uniform(-18/255, 18/255) for hue, each drawn when its op comes up.  The reference's DISTRIBUTION, not its random stream (as
    DeviceMosaicStage.draw_regions).  rng: anything with shuffle and uniform.  -> (order, factors) for photometric_plan."""
    order = [BRIGHTNESS, CONTRAST, SATURATION, HUE]
    rng.shuffle(order)
    factors = {}
    for op in order:
        factors[op] = rng.uniform(-18 / 255., 18 / 255.) if op == HUE else rng.uniform(0.5, 1.5)
    return order, factors


def draw_zoom_out(h, w, max_scale=3, rng=random):
    """zoom_out_'s draws (transforms_.py:134-140) for an h x w frame -> ((new_h, new_w), (top, left)).  The distribution, not the stream."""
    scale = rng.uniform(1, max_scale)
    new_h, new_w = int(scale * h), int(scale * w)
    left = rng.randint(0, new_w - w)
    top = rng.randint(0, new_h - h)
    return (new_h, new_w), (top, left)


def _frame(img, name="img"):
    img = _req(img, torch.uint8, name)
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("%s must be [h, w, 3] uint8 (HWC RGB), got %s" % (name, tuple(img.shape)))
    return img


def photometric_distort(img, plan, out=None):
    """photometric_distort_ for a uint8 HWC frame on the device -> a new uint8 HWC frame.  plan: photometric_plan's array (copied to the
    device here), or an int32[8] DEVICE tensor, which the kernels read when they run: inside a captured graph pass a device tensor and
    write the next draw into it between replays.  No host synchronisation, two launches whatever the plan says."""
    img = _frame(img)
    dev = img.device
    if isinstance(plan, torch.Tensor):
        plan = _req(plan, torch.int32, "plan")
    else:
        plan = torch.from_numpy(np.ascontiguousarray(plan, dtype=np.int32)).to(dev)
    if plan.numel() != 8:
        raise ValueError("plan must hold 8 int32 (four (op, param) slots), got %s" % (tuple(plan.shape),))
    h, w = int(img.shape[0]), int(img.shape[1])
    out = torch.empty_like(img) if out is None else _frame(out, "out")
    if out.shape != img.shape:
        raise ValueError("out must have the shape of img")
    nb = int(lib.frcnn_photometric_workspace(h, w))
    if nb == 0:
        raise ValueError("photometric_distort: unsupported shape %d x %d (sides of 1 .. 32767)" % (h, w))
    ws = _workspace(dev, nb)
    with torch.cuda.device(dev):
        check(lib.frcnn_photometric(_ptr(img), h, w, _ptr(plan), _ptr(out), _ptr(ws), nb, _stream()), "photometric_distort")
    return out


def zoom_out(img, boxes, new_hw, top_left):
    """zoom_out_ for a uint8 HWC frame on the device: -> (canvas uint8 [new_h, new_w, 3] filled with the frame's per-channel median and
    the frame pasted at (top, left); boxes + float32(left, top, left, top), or None for boxes=None).  new_hw and top_left are host
    integers (draw_zoom_out); the histogram and the median never leave the device."""
    img = _frame(img)
    dev = img.device
    h, w = int(img.shape[0]), int(img.shape[1])
    (new_h, new_w), (top, left) = (int(v) for v in new_hw), (int(v) for v in top_left)
    n = 0
    boxes_out = None
    if boxes is not None:
        boxes = _req(boxes, torch.float32, "boxes").reshape(-1, 4)
        n = int(boxes.shape[0])
        boxes_out = torch.empty_like(boxes)
    nb = int(lib.frcnn_zoom_out_workspace(h, w, new_h, new_w))
    if nb == 0:
        raise ValueError("zoom_out: unsupported shapes %d x %d -> %d x %d (sides of 1 .. 32767, the canvas no smaller than the frame)"
                         % (h, w, new_h, new_w))
    canvas = torch.empty((new_h, new_w, 3), dtype=torch.uint8, device=dev)
    ws = _workspace(dev, nb)
    with torch.cuda.device(dev):
        check(lib.frcnn_zoom_out(_ptr(img), h, w, new_h, new_w, top, left, _ptr(boxes) if n else None, n, _ptr(canvas),
                                 _ptr(boxes_out) if n else None, _ptr(ws), nb, _stream()), "zoom_out")
    return canvas, boxes_out


class DeviceAugmentStage:
    """The richer recipe's per-frame chain on the device: [photometric_distort_] -> [zoom_out_] -> DeviceInputStage (flip, resize,
    ToTensor, Normalize, pad).  The reference's recipe (datasets/build.py:28-42) flips BEFORE it zooms out; here the flip is the input
    stage's, behind the zoom-out.  `left` is uniform over its range, and flipping a pasted canvas mirrors the paste position to
    new_w - w - left, which is uniform over the same range: the distribution of results is the same, only the stream of draws is not.

    stage(img_u8_hwc, boxes=None, plan=None, zoom=None, flip=False) -> what DeviceInputStage returns, for the augmented frame.
    plan: None (no photometric distortion), photometric_plan's array or a device int32[8] tensor.  zoom: None or draw_zoom_out's
    ((new_h, new_w), (top, left)).  The coins of RandomPhotoDistortion / RandomZoomOut / RandomHorizontalFlip are the caller's."""

    def __init__(self, size=800, max_size=1333, mean=IMAGENET_MEAN, std=IMAGENET_STD, size_divisible=32, max_scale=3):
        self.final = DeviceInputStage(size, max_size, mean, std, size_divisible)
        self.max_scale = max_scale

    def draw(self, h, w, p_photometric=0.5, p_zoom=0.5, p_flip=0.5, rng=random):
        """The recipe's coins and draws for an h x w frame -> (plan or None, zoom or None, flip)."""
        plan = photometric_plan(*draw_photometric(rng)) if rng.random() < p_photometric else None
        zoom = draw_zoom_out(h, w, self.max_scale, rng) if rng.random() < p_zoom else None
        return plan, zoom, rng.random() < p_flip

    def __call__(self, img, boxes=None, plan=None, zoom=None, flip=False):
        if plan is not None:
            img = photometric_distort(img, plan)
        if zoom is not None:
            img, boxes = zoom_out(img, boxes, zoom[0], zoom[1])
        return self.final(img, boxes, flip)


# ---------------------------------------------------------------------------------------------------------------------------
# crop and the multi-scale crop recipe (new_datasets/transforms.py)
# ---------------------------------------------------------------------------------------------------------------------------
class CropResult(collections.namedtuple("CropResult", "img_u8 boxes labels area iscrowd count")):
    """img_u8 uint8 [ch, cw, 3]; boxes float32 [n, 4], labels int64 [n], area float32 [n] and iscrowd int64 [n] (None when none was
    given) with the first `count` rows live, in input order, and zeros behind them; count int32 [1] on the device."""
    __slots__ = ()

    def to_host(self):
        """What the reference's crop returns: (uint8 array, boxes[:count], labels[:count], area[:count], iscrowd[:count] or None).
        Synchronises."""
        n = int(self.count.item())
        return (self.img_u8.cpu().numpy(), self.boxes[:n].cpu().numpy(), self.labels[:n].cpu().numpy(), self.area[:n].cpu().numpy(),
                None if self.iscrowd is None else self.iscrowd[:n].cpu().numpy())


def crop(img, boxes, labels, region, resize_hw=None, area=None, iscrowd=None, count=None):
    """resize(img, resize_hw) followed by crop(region) (new_datasets/transforms.py:76-132, 16-56) for a uint8 HWC frame on the device,
    without a host read-back -> CropResult.  resize_hw = (H1, W1), None for a plain crop; region = (i, j, h, w) host integers inside the
    resized frame.  boxes float32 [n, 4] pixel xyxy of the SOURCE frame, labels int64 [n], iscrowd int64 [n] or None.  area is accepted
    because the reference's target carries one, and never read: crop replaces every area by that of the clipped box (:33-35).  count:
    None, or a device int32 tensor whose first element says how many leading rows are live (a list an earlier device stage compacted).
    Only the image region is computed; fixed shapes and a device count, so the call can be captured into a graph."""
    img = _frame(img)
    dev = img.device
    h, w = int(img.shape[0]), int(img.shape[1])
    H1, W1 = (h, w) if resize_hw is None else (int(resize_hw[0]), int(resize_hw[1]))
    i, j, ch, cw = (int(v) for v in region)
    boxes = _req(boxes, torch.float32, "boxes").reshape(-1, 4)
    labels = _req(labels, torch.int64, "labels").reshape(-1)
    n = int(boxes.shape[0])
    if iscrowd is not None:
        iscrowd = _req(iscrowd, torch.int64, "iscrowd").reshape(-1)
    for name, t in (("labels", labels), ("area", area), ("iscrowd", iscrowd)):
        if t is not None and int(t.numel()) != n:
            raise ValueError("%s has %d rows, boxes has %d" % (name, int(t.numel()), n))
    if count is not None:
        count = _req(count, torch.int32, "count")
        if count.numel() < 1:
            raise ValueError("count must hold one int32")
    nb = int(lib.frcnn_resize_crop_workspace(h, w, H1, W1, ch, cw)) or 256           # 0: shapes the call itself refuses, and says why
    out = torch.empty((max(ch, 0), max(cw, 0), 3), dtype=torch.uint8, device=dev)
    boxes_out, labels_out = torch.empty_like(boxes), torch.empty_like(labels)
    area_out = torch.empty(n, dtype=torch.float32, device=dev)
    iscrowd_out = None if iscrowd is None else torch.empty_like(iscrowd)
    count_out = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _workspace(dev, nb)
    with torch.cuda.device(dev):
        check(lib.frcnn_resize_crop(_ptr(img), h, w, H1, W1, i, j, ch, cw, _ptr(boxes), _ptr(labels), _ptr(iscrowd), n, _ptr(count), _ptr(out),
                                    _ptr(boxes_out), _ptr(labels_out), _ptr(area_out), _ptr(iscrowd_out), _ptr(count_out), _ptr(ws), nb,
                                    _stream()), "crop")
    return CropResult(out, boxes_out, labels_out, area_out, iscrowd_out, count_out)


def draw_random_crop(h, w, size, rng=random):
    """RandomCrop(size) (transforms.py:162-168) on an h x w frame: torchvision's get_params -- the whole frame when the sizes are equal,
    else the corner uniform over the positions that fit -> (i, j, th, tw).  The reference's DISTRIBUTION, not its random stream
    (get_params draws from torch's generator).  size = (th, tw); rng: anything with randint(a, b), both ends included."""
    th, tw = int(size[0]), int(size[1])
    if th > h or tw > w:
        raise ValueError("a %d x %d crop does not fit a %d x %d frame" % (th, tw, h, w))
    if (h, w) == (th, tw):
        return 0, 0, h, w
    return rng.randint(0, h - th), rng.randint(0, w - tw), th, tw


def draw_random_size_crop(h, w, min_size, max_size, rng=random):
    """RandomSizeCrop(min_size, max_size) (transforms.py:176-180) on an h x w frame: w in [min_size, min(w, max_size)], then h likewise,
    then RandomCrop's corner -> (i, j, ch, cw).  The distribution, not the stream."""
    if min(h, w, max_size) < min_size:
        raise ValueError("a %d x %d frame is smaller than min_size %d" % (h, w, min_size))
    cw = rng.randint(min_size, min(w, max_size))
    ch = rng.randint(min_size, min(h, max_size))
    return draw_random_crop(h, w, (ch, cw), rng)


def center_crop_region(h, w, size):
    """CenterCrop(size) (transforms.py:187-192): size = (crop_h, crop_w); Python's round (half to even) -> (top, left, crop_h, crop_w)."""
    crop_h, crop_w = int(size[0]), int(size[1])
    return int(round((h - crop_h) / 2.)), int(round((w - crop_w) / 2.)), crop_h, crop_w


MultiScalePlan = collections.namedtuple("MultiScalePlan", "flip resize_hw region size")
MultiScalePlan.__doc__ = """flip: the flip coin.  resize_hw, region: None on the plain branch; on the crop branch the (H1, W1) of the
first resize and the (i, j, ch, cw) cropped from it.  size: the scale of the final resize."""


class DeviceMultiScaleStage:
    """The multi-scale recipe of the wired pipeline (sketched in datasets/build.py:27-39), on the device:

        RandomHorizontalFlip, RandomSelect(RandomResize(scales, max_size),
                                           Compose([RandomResize(crop_sizes), RandomSizeCrop(crop_min, crop_max), RandomResize(scales, max_size)]), p),
        ToTensor, Normalize, the pad-to-size_divisible collate

    draw(h, w, rng) -> MultiScalePlan.  stage(img, boxes, labels, plan, area=None, iscrowd=None) -> (x [1, 3, PH, PW] float32, normalised
    boxes [n, 4], labels [n], count int32 [1] on the device, meta).  Rows at and above count are padding, as in DeviceMosaicStage (the
    plain branch keeps every row: count = n).  meta also carries 'area' and 'iscrowd': the crop's on the crop branch, the given ones on the
    plain branch -- in pixels of the frame that enters the final resize (the input stage has no area path; the detector reads neither).
    The recipe flips FIRST; here the flip is the input stage's, behind the crop (as DeviceAugmentStage does for the zoom-out).  The crop's
    corner is uniform over its range and mirroring maps that range onto itself, so the distribution of what is cut out is the same; the
    stream of draws is not, and flipping after the first resize is not the same BYTES as resizing the flipped frame (the resampler's
    22-bit coefficients are not mirror-symmetric to the last bit; neither is the boxes' rounding).  What is pinned is the chain in the
    order run here: resize, crop, hflip, resize, ToTensor, Normalize."""

    def __init__(self, scales, max_size=1333, crop_sizes=(400, 500, 600), crop_min=384, crop_max=600, p=0.5, mean=IMAGENET_MEAN,
                 std=IMAGENET_STD, size_divisible=32):
        self.scales, self.max_size, self.crop_sizes = [int(s) for s in scales], max_size, [int(s) for s in crop_sizes]
        self.crop_min, self.crop_max, self.p = int(crop_min), int(crop_max), float(p)
        self.mean, self.std, self.size_divisible = tuple(mean), tuple(std), size_divisible

    def draw(self, h, w, rng=random, p_flip=0.5):
        """The recipe's coins and draws for an h x w frame, in the recipe's order (the flip coin, RandomSelect's coin, then the branch's own
        draws).  rng: anything with random, choice and randint."""
        flip = rng.random() < p_flip
        if rng.random() < self.p:
            return MultiScalePlan(flip, None, None, rng.choice(self.scales))
        hw1 = get_size((w, h), rng.choice(self.crop_sizes), None)
        region = draw_random_size_crop(hw1[0], hw1[1], self.crop_min, self.crop_max, rng)
        return MultiScalePlan(flip, hw1, region, rng.choice(self.scales))

    def __call__(self, img, boxes, labels, plan, area=None, iscrowd=None):
        final = DeviceInputStage(plan.size, self.max_size, self.mean, self.std, self.size_divisible)
        boxes = _req(boxes, torch.float32, "boxes").reshape(-1, 4)
        if plan.region is None:
            count = torch.full((1,), int(boxes.shape[0]), dtype=torch.int32, device=boxes.device)
        else:
            r = crop(img, boxes, labels, plan.region, plan.resize_hw, area, iscrowd)
            img, boxes, labels, area, iscrowd, count = r
        x, b, meta = final(img, boxes, plan.flip)
        meta["area"], meta["iscrowd"] = area, iscrowd
        return x, b, labels, count, meta
