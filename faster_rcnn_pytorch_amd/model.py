"""VGG16 Faster R-CNN -- host-side mirror of the reference's models/model.py (authoritative variant:
models/model_.py) on top of the HIP hot path.

Same classes, constructor arguments, sub-module names and forward()/predict() signatures as the
reference (models/model.py:12-402), so train.py:31 / test.py:60 work unchanged:
    FRCNN(num_classes).forward(x, bbox, label)
        -> (rpn_cls[1,N,2], rpn_reg[1,N,4], head_cls[R,C], head_reg[R,4]),
           (tgt_rpn_cls[N] i64, tgt_rpn_reg[N,4], tgt_cls[R] i64, tgt_reg[R,4])
    FRCNN.predict(x, opts | threshold) -> (bbox[M,4] f32, label[M] i32, score[M] f32)

What changed underneath (each step cites the reference lines it replaces):
  * anchors: cached in HBM per image shape / regenerated in registers (model.py:310-312 numpy + H2D)
  * RegionProposal: one enqueue of 5 HIP kernels, fixed-capacity output + device count
    (model.py:17-58: ~20 launches, 3 host syncs, torchvision nms with a host scan)
  * target makers: 3 + 1 HIP kernels, sampling by device Philox keys (model.py:127-266: ~45 launches,
    7-9 host syncs, CPU randperm).  sampling='host' reproduces the reference's RNG stream exactly
    (torch.randperm on the CPU generator, RPN maker first: SURVEY Q4) at the price of the same syncs.
  * RoIPool: HIP forward/backward (torchvision.ops.RoIPool, model.py:97,113)
  * RPN head: the 3x3 convolution on the fp32 matrix cores (Winograd stage, csrc/rpn_conv_f32.hip), bias + ReLU + both 1x1 heads + the
    NHWC layout in one more MFMA kernel (csrc/rpn_head.hip) (model.py:68-83: three MIOpen calls + two transposing copies)
  * extractor: its thirteen stride-1 3x3 convolutions run on the same fp32 stage, each with the ReLU (and, where the 4 x 4 tile is used,
    the 2 x 2 max-pool) behind it in the same call (VGGExtractor below; csrc/conv_c3.hip for the three-channel first layer).  Layers the
    stage does not take (autocast, batch > 1) run as the torch modules they are.
The FC head (classifier / cls_head / reg_head), the optimizer and the loss's reductions over torch tensors stay on PyTorch-ROCm (hipBLASLt).
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .anchor import FRCNNAnchorMaker


def _unwrap(t):
    """bbox/label calling convention: a list with one tensor (model_.py:130-131,188) or a bare tensor (train.py:18-19)."""
    return t[0] if isinstance(t, (list, tuple)) else t


def normal_init(m, mean, stddev):
    m.weight.data.normal_(mean, stddev)
    m.bias.data.zero_()


def vgg16_features():
    """torchvision.models.vgg16().features with identical layer indices (state_dict keys extractor.N.*);
    random init here: pretrained weights need the network."""
    cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
    layers, c_in = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(c_in, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            c_in = v
    for m in layers:
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(m.bias, 0)
    return layers


class VGGExtractor(nn.Sequential):
    """`nn.Sequential(*list(vgg16.features)[:-1])` (models/model.py:279-281) with the same children, indices and state_dict keys.  Its forward walks
    the children like nn.Sequential does, except that a 3x3 convolution the fp32 Winograd stage takes (ops.conv3x3_supported: 128-multiples of
    channels, batch 1, fp32 on the device) runs there TOGETHER with the ReLU behind it -- bias and ReLU in the output transform, the ReLU's
    backward in the gradient kernels' transforms -- instead of three vendor / elementwise launches forward and four backward; a 2 x 2 max-pool
    behind such a pair joins the same call where the stage uses its 4 x 4 tile; the first convolution (three input channels) has kernels of
    its own.  Every other child (small maps' pools; any layer under autocast or with batch > 1) runs as it is."""

    def forward(self, x):
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.padding == (1, 1) and m.stride == (1, 1) and m.dilation == (1, 1)
                    and m.groups == 1 and m.bias is not None and not torch.is_autocast_enabled() and ops.conv3x3_supported(x, m.weight)):
                fuse = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                p = mods[i + 2] if fuse and i + 2 < len(mods) else None
                pool = (isinstance(p, nn.MaxPool2d) and p.kernel_size in (2, (2, 2)) and p.stride in (2, (2, 2)) and p.padding in (0, (0, 0))
                        and p.dilation in (1, (1, 1)) and not p.ceil_mode and not p.return_indices and ops.conv3x3_pool_supported(x))
                x = ops.conv3x3(x, m.weight, m.bias, relu=fuse, pool=pool)      # conv + ReLU (+ the 2 x 2 max-pool behind it) in one stage call
                i += 3 if pool else (2 if fuse else 1)
                continue
            if (isinstance(m, nn.Conv2d) and m.in_channels == 3 and m.kernel_size == (3, 3) and m.padding == (1, 1) and m.stride == (1, 1)
                    and m.dilation == (1, 1) and m.groups == 1 and not torch.is_autocast_enabled() and ops.conv3x3_c3_supported(x, m.weight)):
                fuse = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                x = ops.conv3x3_c3(x, m.weight, m.bias, relu=fuse)              # features[0] (+ [1]): three input channels, a byte mover (csrc/conv_c3.hip)
                i += 2 if fuse else 1
                continue
            x = m(x)
            i += 1
        return x


class RegionProposal(nn.Module):
    """models/model.py:12-58."""

    def __init__(self):
        super().__init__()
        self.min_size = 1
        self.nms_threshold = 0.7

    @staticmethod
    def top_k(mode):
        return (6000, 300) if mode == "test" else (12000, 2000)              # model.py:24-28

    def propose(self, cls, reg, anchor, mode, grid=None, want_src=False):
        """Asynchronous form: (rois [P,4] fixed capacity, count int32[1] on device, src | None)."""
        pre, post = self.top_k(mode)
        return ops.region_proposal(reg.detach().float(), cls.detach().float(), anchor, self.min_size / 1000, pre, self.nms_threshold, post,
                                   grid=grid, want_src=want_src)

    def forward(self, cls, reg, anchor, mode):
        """Reference signature: returns roi_tensor [n,4] (variable length -> one host sync for n)."""
        rois, cnt, _ = self.propose(cls, reg, anchor, mode)
        return rois[:ops.host_count(cnt, 'region_proposal')]


class _RPNHead(nn.Module):
    """The three convolutions of both mirrors' RPN heads and their reference form (models/model.py:68-83, models/new_model.py:96-113)."""

    def __init__(self, in_channels, out_channels, num_anchors):
        super().__init__()
        self.inter_layer = nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1)
        self.cls_layer = nn.Conv2d(in_channels, num_anchors * 2, kernel_size=1)
        self.reg_layer = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=1)
        normal_init(self.inter_layer, 0, 0.01)
        normal_init(self.cls_layer, 0, 0.01)
        normal_init(self.reg_layer, 0, 0.01)

    def forward(self, features):
        batch_size = features.size(0)
        x = torch.relu(self.inter_layer(features))
        pred_cls = self.cls_layer(x)
        pred_reg = self.reg_layer(x)
        pred_reg = pred_reg.permute(0, 2, 3, 1).contiguous().view(batch_size, -1, 4)
        pred_cls = pred_cls.permute(0, 2, 3, 1).contiguous().view(batch_size, -1, 2)
        return pred_cls, pred_reg


class RegionProposalNetwork(_RPNHead):
    """models/model.py:61-84."""

    def __init__(self, in_channels=512, out_channels=512):
        super().__init__(in_channels, out_channels, num_anchors=9)

    def forward(self, features):
        if (features.is_cuda and features.dtype == torch.float32 and features.size(0) == 1 and not torch.is_autocast_enabled()
                and ops.rpn_conv3x3_supported([features], self.inter_layer.weight)):
            # the 3x3 without its bias on the fp32 matrix cores (csrc/rpn_conv_f32.hip: forward, data and weight gradient hand-written);
            # bias + ReLU + both 1x1 heads + the NHWC layout in one more MFMA kernel
            raw = ops.rpn_conv3x3([features], self.inter_layer.weight)[0]
            return ops.rpn_head_tail(raw, self.inter_layer.bias, self.cls_layer.weight, self.cls_layer.bias,
                                     self.reg_layer.weight, self.reg_layer.bias)
        return super().forward(features)                                           # reference form (autocast / batch > 1)


class FastRCNNHead(nn.Module):
    """models/model.py:87-120."""

    def __init__(self, num_classes, roi_size, classifier):
        super().__init__()
        self.num_classes = num_classes
        self.cls_head = nn.Linear(4096, num_classes)
        self.reg_head = nn.Linear(4096, num_classes * 4)
        self.roi_pool = ops.RoIPool(output_size=(roi_size, roi_size), spatial_scale=1.)
        self.classifier = classifier
        normal_init(self.cls_head, 0, 0.01)
        normal_init(self.reg_head, 0, 0.001)

    def forward(self, features, roi):
        f_height, f_width = features.size()[2:]
        scale = ops.const_tensor((f_width, f_height, f_width, f_height), roi.device)   # cached: torch.tensor(list, device=cuda) is a blocking copy
        scaled_roi = roi * scale                                               # model.py:107-109
        pool = self.roi_pool(features.float(), [scaled_roi])           # the hot path computes in fp32 (also under autocast)
        x = pool.view(pool.size(0), -1)
        x = self.classifier(x)
        return self.cls_head(x), self.reg_head(x)


class _Sampler(object):
    """Sampling policy shared by the two target makers."""

    def __init__(self, sampling="device", seed=0):
        if sampling not in ("device", "host"):
            raise ValueError("sampling must be 'device' (Philox on the GPU, no sync) or 'host' (reference RNG stream)")
        self.sampling = sampling
        self.seed = int(seed)
        # sticky device-side error word: the sync-free ('device') target makers OR their failure bits into it; the training
        # loop reads it where it syncs anyway (FRCNN.check_device_status()).  The same failures also make the loss NaN.
        self.status = ops.DeviceStatus()
        self._state = {}

    def state(self, device):
        """The device-resident Philox stream (seed, offset) of this model on `device`: each target-maker call uses the pair it
        finds and leaves offset + 1 behind, ON THE DEVICE -- no host-side counter rides in the launch arguments, so the whole
        step can be captured in a HIP graph and still draws fresh samples at every replay."""
        key = str(device)
        st = self._state.get(key)
        if st is None:
            st = ops.philox_state(self.seed, 1, device)
            self._state[key] = st
        return st

    def reseed(self, seed=None, offset=1):
        """Restart the stream (tests; deterministic replays): a device-side copy into the existing state tensors, no sync."""
        if seed is not None:
            self.seed = int(seed)
        for key, st in self._state.items():
            st.copy_(ops.philox_state(self.seed, offset, st.device))


class FastRcnnTargetMaker(nn.Module):
    """models/model_.py:123-179.  The FPN mirror's head target maker is this one with other constants (ops.head_targets) and its own
    reference line in the short-sample message."""
    variant, label_offset, max_pos, total = 0, 1, 32, 128
    cite = "the reference fails here too, model_.py:340"

    def __init__(self, sampler=None):
        super().__init__()
        self.sampler = sampler or _Sampler()

    def forward(self, bbox, label, rois, n_rois=None, n_gt=None, empty=None):
        """n_gt (device int32): bbox / label are fixed-capacity lists with n_gt live rows (ops.head_targets); empty: see there."""
        bbox = _unwrap(bbox)
        label = _unwrap(label).to(torch.int64)
        s = self.sampler
        kw = dict(n_rois=n_rois, variant=self.variant, label_offset=self.label_offset, max_pos=self.max_pos, total=self.total, n_gt=n_gt)
        if s.sampling == "host":
            c = ops.head_targets(rois, bbox, label, **kw)[4].cpu().tolist()                # learn the candidate counts
            perm_pos = torch.randperm(c[0])                                                # model_.py:149, new_model.py:175
            perm_neg = torch.randperm(c[1])                                                # model_.py:155, new_model.py:180
            cls, reg, srois, _, counts = ops.head_targets(rois, bbox, label, perm_pos=perm_pos, perm_neg=perm_neg, empty=empty, **kw)
            if counts.cpu().tolist()[2] != self.total:
                raise RuntimeError("%s: fewer than %d samples (%s)" % (type(self).__name__, self.total, self.cite))
        else:
            cls, reg, srois, _, _ = ops.head_targets(rois, bbox, label, philox_state=s.state(rois.device),
                                                     status=s.status.word(rois.device), empty=empty, **kw)
        return cls, reg, srois


class RPNTargetMaker(nn.Module):
    """models/model_.py:182-266.  The FPN mirror's RPN target maker is this one with variant = 1 (ops.rpn_targets)."""
    variant = 0

    def __init__(self, sampler=None):
        super().__init__()
        self.sampler = sampler or _Sampler()

    def forward(self, bbox, anchor, n_gt=None):
        """n_gt (device int32): bbox is a fixed-capacity list with n_gt live rows (ops.rpn_targets)."""
        bbox = _unwrap(bbox)
        s = self.sampler
        if s.sampling == "host":
            n_pos, n_neg = ops.rpn_targets(anchor, bbox, variant=self.variant, n_gt=n_gt)[2].cpu().tolist()[:2]
            perm_pos = torch.randperm(n_pos) if n_pos > 128 else None                      # model_.py:225-229
            perm_neg = torch.randperm(n_neg) if n_neg > 256 - n_pos else None              # model_.py:231-236
            cls, reg, counts = ops.rpn_targets(anchor, bbox, variant=self.variant, perm_pos=perm_pos, perm_neg=perm_neg, n_gt=n_gt)
            err = counts.cpu().tolist()[2]
            if err & ~ops._lib.RPN_ERR_GT_COUNT:
                raise RuntimeError("RPNTargetMaker: permutation length mismatch")
            if err:
                raise RuntimeError("RPNTargetMaker: n_gt outside [1, %d]" % bbox.shape[0])
        else:
            cls, reg, _ = ops.rpn_targets(anchor, bbox, variant=self.variant, philox_state=s.state(anchor.device), n_gt=n_gt)
        return cls, reg


class _Detector(nn.Module):
    """What the two FRCNN mirrors share, and the interface parallel.GraphStep / FrameSlot, inference.DetectGraph and bench.py rely on:
    forward(x, boxes, labels, n_gt=, empty=), predict, detect, proposals, graph_stages(), check_device_status(), and the attributes num_classes,
    sampler and last_proposal_count.  A mirror writes forward and graph_stages itself and gives predict / detect two hooks:
        _test_proposals(x)         -> (features, rois [P,4] fixed capacity, n_rois device int32[1]), test mode, no host sync
        _head(features, rois, x)   -> (head_cls [R,C], head_reg [R,4C])"""

    def count_parameters(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def check_device_status(self):
        """Raises if a device-side failure was recorded since the last call (an aborted NMS scan upstream of the head target
        maker, or fewer than 128 / 512 RoI samples -- where the reference throws, model.py:340, or asserts, new_model.py:182).  One
        host sync: call it at the logging / checkpoint interval.  The same failures turn the step's loss into NaN, so a caller that
        prints loss.item() sees them even without this call."""
        self.sampler.status.check()

    @staticmethod
    def _target_class_rows(pred_reg, target_cls, rows):
        """models/model.py:340-341 in both mirrors: row i of the `rows` sampled RoIs keeps the regression of its target class (reference:
        pred[arange(rows), cls], advanced indexing).  torch.gather selects the same elements with one kernel forward and one backward;
        the indexing form costs an arange, an index kernel and a rocprim sort + scatter in backward (~30 us and 7 launches per step)."""
        idx = target_cls.clamp(min=0).view(-1, 1, 1).expand(-1, 1, 4)             # (-1 = unsampled row: its loss is NaN anyway)
        return torch.gather(pred_reg.reshape(rows, -1, 4), 1, idx).squeeze(1)

    def _decode(self, rois, head_cls, head_reg):
        """models/model.py:369-378, models/new_model.py:437-445: (clamped boxes [R, 4C], probabilities [R, C]) of the live RoIs."""
        pred_cls = torch.softmax(head_cls, dim=-1)                               # model.py:369
        head_reg = head_reg.reshape(-1, self.num_classes, 4) * ops.const_tensor((0.1, 0.1, 0.2, 0.2), head_reg.device)   # model.py:372
        rois = rois.reshape(-1, 1, 4).expand_as(head_reg)
        pred_bbox = ops.cxcy_to_xy(ops.decode(head_reg.reshape(-1, 4).contiguous(), ops.xy_to_cxcy(rois.reshape(-1, 4).contiguous())))
        return pred_bbox.reshape(-1, self.num_classes * 4).clamp(min=0, max=1), pred_cls

    @torch.no_grad()
    def predict(self, x, opts):
        """opts: an object with .thres (model.py:346) or a bare float threshold (model_.py:346)."""
        threshold = float(getattr(opts, "thres", opts))
        features, rois, n_rois = self._test_proposals(x)
        rois = rois[:ops.host_count(n_rois, 'region_proposal')]
        head_cls, head_reg = self._head(features, rois, x)
        return self._suppress(*self._decode(rois, head_cls, head_reg), threshold)

    @staticmethod
    def _proposal_detections(rois, n_rois):
        """The fixed-capacity RoIs as an ops.Detections for evaluation.ProposalEvaluator: labels 0, count = n_rois, and scores[i] =
        float32(P - i) -- the proposals leave NMS in objectness order, so the exact, strictly descending ramp restates their rank; only the
        order is used."""
        P = rois.shape[0]
        ramp = torch.arange(P, 0, -1, dtype=torch.float32, device=rois.device)
        return ops.Detections(rois, torch.zeros(P, dtype=torch.int32, device=rois.device), ramp, n_rois, None, None, n_rois)

    @torch.no_grad()
    def proposals(self, x):
        """The test-mode proposals of _test_proposals as an ops.Detections (boxes = the fixed-capacity RoIs, labels = 0, scores = a rank
        ramp, count = the device count), with no host sync: what evaluation.ProposalEvaluator.update takes."""
        _, rois, n_rois = self._test_proposals(x)
        return self._proposal_detections(rois, n_rois)

    @torch.no_grad()
    def detect(self, x, opts_or_threshold, threshold_dev=None, want_prob=False, want_proposals=False, soft_nms=None):
        """predict without a host sync (graph-capturable): the test-mode path with the fixed-capacity proposals and their device count,
        the head on all P rows, and the post-processing of models/model.py:368-402 / models/new_model.py:420-470 in
        ops.detect_postprocess.  threshold_dev (a device float32[1]) overrides the threshold when given.  Returns ops.Detections (its
        n_rois is the proposal count); .to_host() gives what predict returns.  want_proposals=True returns (detections, proposals), the
        second as proposals(x) gives them: one forward serves both evaluators.
        soft_nms (an ops.SoftNMS; None = the above, unchanged): the per-class suppression becomes Soft-NMS at the same 0.3.  The
        post-process runs with nms_threshold = +inf -- nothing exceeds it, so every thresholded candidate comes out, class-major and in
        score order -- and ops.merge_detections of that one set does the suppression; the result is an ops.MergedDetections (decayed
        scores, a status word) that carries prob and n_rois through."""
        threshold = float(getattr(opts_or_threshold, "thres", opts_or_threshold))
        features, rois, n_rois = self._test_proposals(x)
        head_cls, head_reg = self._head(features, rois, x)                        # rows >= n_rois: zero boxes, ignored below
        if soft_nms is None:
            dets = ops.detect_postprocess(head_cls, head_reg, rois, n_rois, threshold, 0.3, threshold_dev=threshold_dev, want_prob=want_prob)
        else:
            dets = self._soft_suppress(self._candidates(head_cls, head_reg, rois, n_rois, threshold, threshold_dev, want_prob), soft_nms)
        return (dets, self._proposal_detections(rois, n_rois)) if want_proposals else dets

    @staticmethod
    def _candidates(head_cls, head_reg, rois, n_rois, threshold, threshold_dev, want_prob=False):
        """Every thresholded candidate of the head outputs, unsuppressed: the post-process at nms_threshold = +inf."""
        return ops.detect_postprocess(head_cls, head_reg, rois, n_rois, threshold, float("inf"), threshold_dev=threshold_dev, want_prob=want_prob)

    def _soft_suppress(self, cands, soft_nms):
        out = ops.merge_detections([cands], num_classes=self.num_classes, min_score=float("-inf"), nms_threshold=0.3, soft_nms=soft_nms)
        return ops.MergedDetections(out.boxes, out.labels, out.scores, out.count, out.class_counts, cands.prob, cands.n_rois, out.status)

    @torch.no_grad()
    def detect_tta(self, views, threshold, threshold_dev=None, nms_threshold=0.3, vote_threshold=None, soft_nms=None):
        """Test-time augmentation without a host sync (graph-capturable): detect on every view, one after the other on the current
        stream, then ops.merge_detections.  views: one tensor x, which stands for the two views x and x.flip(-1), or a list of
        (x_k, mirrored) pairs of any input size each -- mirrored=True says x_k is the frame flipped horizontally, so its boxes are
        mirrored back; normalised boxes need nothing else across scales.  The merge takes every detection of the views (their scores
        passed `threshold` already), suppresses per class at nms_threshold and, with vote_threshold, replaces every kept box by the
        score-weighted mean of the candidates that overlap it that much.  Returns ops.MergedDetections.
        soft_nms (an ops.SoftNMS; None = the above, unchanged): every view contributes its UNSUPPRESSED thresholded candidates and the
        merge's Soft-NMS scan (decay threshold nms_threshold) is the only suppression -- Detectron's order of operations.  This raises
        the per-class candidate count to as many as K views x P RoIs against the merge's limit of 2048 per class; a class above it
        comes out empty with count = -1 and MERGE_CLASS_OVERFLOW in the status word, as ever."""
        if isinstance(views, torch.Tensor):
            views = [(views, False), (views.flip(-1), True)]
        views = list(views)
        if soft_nms is None:
            sets = [self.detect(x, threshold, threshold_dev=threshold_dev) for x, _ in views]
        else:
            sets = []
            for x, _ in views:
                features, rois, n_rois = self._test_proposals(x)
                head_cls, head_reg = self._head(features, rois, x)
                sets.append(self._candidates(head_cls, head_reg, rois, n_rois, float(getattr(threshold, "thres", threshold)), threshold_dev))
        return ops.merge_detections(sets, hflip=[bool(f) for _, f in views], num_classes=self.num_classes, min_score=float("-inf"),
                                    nms_threshold=nms_threshold, vote_threshold=vote_threshold, soft_nms=soft_nms)

    def _suppress(self, raw_cls_bbox, raw_prob, threshold):
        """models/model.py:382-402 (per-class score mask + nms(0.3), class 0 = background skipped, results concatenated
        class by class) as ONE class-aware NMS: 2 host syncs in total instead of 2 per class."""
        R = raw_prob.shape[0]
        boxes = raw_cls_bbox.reshape((R, self.num_classes, 4))[:, 1:, :]
        prob = raw_prob[:, 1:]
        ridx, cidx = (prob > threshold).nonzero(as_tuple=True)                    # sync 1: number of candidates
        cand_box = boxes[ridx, cidx].contiguous()
        cand_score = prob[ridx, cidx].contiguous()
        keep = ops.batched_nms(cand_box, cand_score, cidx, 0.3)                   # sync 2: number kept (score-descending)
        bbox = cand_box[keep].cpu().numpy()
        label = cidx[keep].cpu().numpy()                                          # 0-based: l - 1 in the reference
        score = cand_score[keep].cpu().numpy()
        order = np.argsort(label, kind="stable")                                  # class-major, score-descending inside a class
        bbox = torch.from_numpy(bbox[order].astype(np.float32))
        label = torch.from_numpy(label[order].astype(np.int32))
        score = torch.from_numpy(score[order].astype(np.float32))
        return bbox, label, score


class FRCNN(_Detector):
    """models/model.py:269-402 (VGG16 Faster R-CNN)."""

    def __init__(self, num_classes=81, pretrained=False, sampling="device", seed=0):
        super().__init__()
        if pretrained:
            raise RuntimeError("pretrained weights need the network (gdown / torchvision hub); load a state_dict instead")
        self.num_classes = num_classes
        self.extractor = VGGExtractor(*vgg16_features()[:-1])                  # model.py:279-281: drop the last max-pool
        self.classifier = nn.Sequential(nn.Linear(in_features=25088, out_features=4096), nn.ReLU(inplace=True),
                                        nn.Linear(in_features=4096, out_features=4096), nn.ReLU(inplace=True))
        self.sampler = _Sampler(sampling, seed)
        self.rpn = RegionProposalNetwork()
        self.rp = RegionProposal()
        self.anchor_maker = FRCNNAnchorMaker()
        self.rpn_target_maker = RPNTargetMaker(self.sampler)
        self.fast_rcnn_target_maker = FastRcnnTargetMaker(self.sampler)
        self.fast_rcnn_head = FastRCNNHead(num_classes=num_classes, roi_size=7, classifier=self.classifier)
        self.last_proposal_count = None

    def graph_stages(self):
        """Where parallel.GraphStep cuts the backward: everything behind the RoI pooling (the FC head: 120 M of the 137 M parameters) has its
        gradient first, and its all-reduce runs under the backward of the rest."""
        return {"cut_module": self.fast_rcnn_head.roi_pool, "late_modules": (self.classifier, self.fast_rcnn_head.cls_head, self.fast_rcnn_head.reg_head)}

    def forward(self, x, bbox, label, n_gt=None, empty=None):
        """n_gt (device int32[1]): bbox / label come as fixed-capacity lists straight from the device input stage, rows at and above
        n_gt are padding; the target makers read the count on the device, so nothing about the number of boxes is frozen into a captured
        step (parallel.FrameSlot).  empty (device int32[1]): set to 1 by a frame without boxes, else 0 -- DeviceSGD's guard= tensor."""
        hw = x.size()[2:]
        # 5. rpn targets depend only on the anchors and the ground truth (model.py:324), not on the network: they are enqueued first.
        #    (Round 1 ran them on a second HIP stream "underneath" the backbone.  Measured A/B on one box, four runs: the fork / join
        #    and the single-workgroup sampler competing with MIOpen's kernels cost more than the 48 us they hide: 14.77-14.80 ms per step
        #    with the side stream, 14.63-14.67 ms without; the same experiment in the FPN mirror: 18.64 vs 18.17 ms.)
        anchor = self.anchor_maker.device_anchors(hw, x.device)           # model.py:310-312: resident in HBM
        target_rpn_cls, target_rpn_reg = self.rpn_target_maker(bbox=bbox, anchor=anchor, n_gt=n_gt)
        # 1. extract features                                                  model.py:307
        features = self.extractor(x)
        # 3. forward rpn                                                       model.py:315
        pred_rpn_cls, pred_rpn_reg = self.rpn(features)
        # 4. propose regions -> fixed-capacity rois + device count (anchors regenerated in registers)   model.py:318
        rois, n_rois, _ = self.rp.propose(pred_rpn_cls.squeeze(0), pred_rpn_reg.squeeze(0), None, "train",
                                          grid=self.anchor_maker.grid_desc(hw))
        self.last_proposal_count = n_rois                                     # device int32[1]: how many proposals survived NMS (<= 2000)
        # 6. fast rcnn targets                                                 model.py:328
        target_fast_rcnn_cls, target_fast_rcnn_reg, sample_rois = self.fast_rcnn_target_maker(bbox=bbox, label=label, rois=rois,
                                                                                              n_rois=n_rois, n_gt=n_gt, empty=empty)
        # 7. fast rcnn head                                                    model.py:335
        pred_fast_rcnn_cls, pred_fast_rcnn_reg = self.fast_rcnn_head(features, sample_rois)
        # 8. regression row of the target class                                model.py:340-341
        pred_fast_rcnn_reg = self._target_class_rows(pred_fast_rcnn_reg, target_fast_rcnn_cls, 128)
        return (pred_rpn_cls, pred_rpn_reg, pred_fast_rcnn_cls, pred_fast_rcnn_reg), \
               (target_rpn_cls, target_rpn_reg, target_fast_rcnn_cls, target_fast_rcnn_reg)

    def _test_proposals(self, x):
        features = self.extractor(x)
        pred_rpn_cls, pred_rpn_reg = self.rpn(features)
        rois, n_rois, _ = self.rp.propose(pred_rpn_cls.squeeze(0), pred_rpn_reg.squeeze(0), None, "test",
                                          grid=self.anchor_maker.grid_desc(x.size()[2:]))
        return features, rois, n_rois

    def _head(self, features, rois, x):
        return self.fast_rcnn_head(features, rois)


def build_model(opts=None, num_classes=21, device=None, **kw):
    """models/build.py:7-19: construct, move to the device, wrap in DDP when torch.distributed is initialised."""
    from .parallel import wrap_ddp
    num_classes = getattr(opts, "num_classes", num_classes) if opts is not None else num_classes
    model = FRCNN(num_classes=num_classes, **kw)
    if device is not None:
        model = model.to(device)
        model = wrap_ddp(model, torch.device(device))
    return model
