"""Graph-captured inference: FRCNN.detect (both mirrors) recorded once into a HIP graph and replayed per frame.

The test loop of the reference (test.py:60) calls predict once per image; every call pays the Python launch cost of the whole
network.  DetectGraph records detect -- which has no host sync -- for one input size and replays it."""
import torch


class DetectGraph(object):
    """model.detect at a fixed [1, 3, H, W] input size, captured into one torch.cuda.graph.

    __call__(x) copies x into the graph's static input buffer, replays, and returns the graph's static ops.Detections: its tensors are
    overwritten by the next call (clone them, or call .to_host(), to keep a result).  The score threshold lives in a device tensor
    that the kernels read at replay time, so set_threshold() takes effect on the next call without a new capture.

    evaluator= (an evaluation.DetectionEvaluator with gt= an evaluation.GroundTruth for the VOC protocol, or an
    evaluation.CocoDetectionEvaluator with gt= an evaluation.CocoGroundTruth for the COCO one) adds the evaluator's per-frame update to the same
    graph: the reference's test loop (test.py:60: predict, then the evaluator) as one replay per frame with no host sync.  Write the
    frame's ground truth with gt.set(...) before the call (the warm-up and the capture score nothing).  Without them the captured
    graph is detect alone.

    proposal_evaluator= (an evaluation.ProposalEvaluator, or any CocoDetectionEvaluator(use_cats=False), with gt= an
    evaluation.CocoGroundTruth) also scores the frame's proposals -- the same forward's RoIs, model.detect(..., want_proposals=True) -- in
    the same graph, with or without evaluator=.  self.proposals is then the graph's static proposal Detections.

    soft_nms= (an ops.SoftNMS) is handed to model.detect: the captured suppression is Soft-NMS and the static result an
    ops.MergedDetections; the evaluators take it unchanged."""

    def __init__(self, model, image_hw, threshold=0.05, device=None, warmup=2, evaluator=None, gt=None, proposal_evaluator=None, soft_nms=None):
        m = getattr(model, "module", model)                     # a DDP-wrapped model: capture the module itself
        dev = torch.device(device) if device is not None else next(m.parameters()).device
        H, W = (int(v) for v in image_hw)
        if (evaluator is None and proposal_evaluator is None) != (gt is None):
            raise ValueError("DetectGraph: evaluator= and gt= go together")
        self.model = m
        self.evaluator, self.gt, self.proposal_evaluator = evaluator, gt, proposal_evaluator
        self.proposals = None
        want = proposal_evaluator is not None

        def detect():
            kw = {} if soft_nms is None else {"soft_nms": soft_nms}
            if not want:
                return m.detect(self.x, float(threshold), threshold_dev=self.threshold, **kw), None
            return m.detect(self.x, float(threshold), threshold_dev=self.threshold, want_proposals=True, **kw)
        self.image_hw = (H, W)
        self.x = torch.zeros((1, 3, H, W), dtype=torch.float32, device=dev)
        self.threshold = torch.full((1,), float(threshold), dtype=torch.float32, device=dev)
        # eager warm-up on a side stream: lazy allocations, cached constants and anchor grids, workspaces
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(int(warmup), 1)):
                out, props = detect()
            if evaluator is not None:
                evaluator._workspace(out.labels.numel(), gt.capacity)         # the update's zeroed workspace: allocated outside the capture
            if want:
                proposal_evaluator._workspace(props.labels.numel(), gt.capacity)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out, self.proposals = detect()
            if evaluator is not None:
                evaluator.update(self.out, gt)
            if want:
                proposal_evaluator.update(self.proposals, gt)

    def set_threshold(self, t):
        """Writes the device threshold in place: the next replay uses it."""
        self.threshold.fill_(float(t))

    def __call__(self, x):
        if tuple(x.shape) != tuple(self.x.shape):
            raise ValueError("DetectGraph: captured for input %s, got %s" % (tuple(self.x.shape), tuple(x.shape)))
        self.x.copy_(x)
        self.graph.replay()
        return self.out


class TTADetectGraph(object):
    """model.detect_tta at fixed input sizes, captured into one torch.cuda.graph: one static [1, 3, H, W] input per entry of view_hws, the
    mirrored copy of each (hflip=True) made inside the graph, detect on every view one after the other on the capture stream -- no side
    streams, so the graph is one chain -- the merge of the views' detections (ops.merge_detections; vote_threshold=None leaves box voting
    off) and, with evaluator= and gt= as in DetectGraph, the evaluator's update on the MERGED set.

    __call__(xs) takes one frame per size (a single tensor when there is one size), copies each into its static buffer, replays, and
    returns the graph's static ops.MergedDetections: overwritten by the next call.  set_threshold() works as in DetectGraph: the views'
    score threshold is a device tensor read at replay time.  soft_nms= (an ops.SoftNMS) is handed to model.detect_tta: the views
    contribute their unsuppressed candidates and the merge's Soft-NMS scan is the only suppression."""

    def __init__(self, model, view_hws, hflip=True, threshold=0.05, nms_threshold=0.3, vote_threshold=None, evaluator=None, gt=None, device=None,
                 warmup=2, soft_nms=None):
        m = getattr(model, "module", model)                     # a DDP-wrapped model: capture the module itself
        dev = torch.device(device) if device is not None else next(m.parameters()).device
        view_hws = list(view_hws)
        if view_hws and isinstance(view_hws[0], int):            # one (H, W)
            view_hws = [tuple(view_hws)]
        self.view_hws = [(int(h), int(w)) for h, w in view_hws]
        if not self.view_hws:
            raise ValueError("TTADetectGraph: no view size")
        if (evaluator is None) != (gt is None):
            raise ValueError("TTADetectGraph: evaluator= and gt= go together")
        self.model, self.evaluator, self.gt, self.hflip = m, evaluator, gt, bool(hflip)
        self.xs = [torch.zeros((1, 3, h, w), dtype=torch.float32, device=dev) for h, w in self.view_hws]
        self.threshold = torch.full((1,), float(threshold), dtype=torch.float32, device=dev)

        def detect():
            views = []
            for x in self.xs:
                views.append((x, False))
                if self.hflip:
                    views.append((x.flip(-1), True))
            kw = {} if soft_nms is None else {"soft_nms": soft_nms}
            return m.detect_tta(views, float(threshold), threshold_dev=self.threshold, nms_threshold=nms_threshold, vote_threshold=vote_threshold, **kw)
        # eager warm-up on a side stream, as DetectGraph: lazy allocations, cached constants and anchor grids, workspaces
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(int(warmup), 1)):
                out = detect()
            if evaluator is not None:
                evaluator._workspace(out.labels.numel(), gt.capacity)             # the update's zeroed workspace: allocated outside the capture
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = detect()
            if evaluator is not None:
                evaluator.update(self.out, gt)

    def set_threshold(self, t):
        """Writes the device threshold in place: the next replay uses it."""
        self.threshold.fill_(float(t))

    def __call__(self, xs):
        xs = [xs] if isinstance(xs, torch.Tensor) else list(xs)
        if len(xs) != len(self.xs) or any(tuple(x.shape) != tuple(b.shape) for x, b in zip(xs, self.xs)):
            raise ValueError("TTADetectGraph: captured for inputs %s, got %s" % ([tuple(b.shape) for b in self.xs], [tuple(x.shape) for x in xs]))
        for x, b in zip(xs, self.xs):
            b.copy_(x)
        self.graph.replay()
        return self.out
