"""Data-parallel plumbing: one process per GPU, torch.distributed (backend 'nccl' == RCCL on ROCm)
over xGMI; mirrors the reference's utils/__init__.py:5-25 (init) and models/build.py:7-19 (DDP wrap).

The proposal / RoI path shards naturally (one image per GPU, no exchange); the only steady-state
collective is DDP's bucketed gradient all-reduce, overlapped with backward.  Bucket size: the VGG16
gradient is 548 MB fp32 and xGMI is point-to-point (per-link bound ring), so larger buckets than
DDP's 25 MB default amortise the per-collective latency; classifier.0 (411 MB) finishes its backward
first, which lets its reduction overlap the whole conv backward.
"""
import gc
import os

import torch
import torch.distributed as dist


def dist_env():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def init_for_distributed(backend=None):
    """Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torchrun).  Returns (rank, local_rank, world, device)."""
    rank, local_rank, world = dist_env()
    use_cuda = torch.cuda.is_available()
    if backend is None:
        # FRCNN_DIST_BACKEND=gloo: rehearsal of the N > 1 code path where RCCL cannot run (several ranks sharing the one GPU of a test box:
        # RCCL refuses two ranks on one device); never set in a measured run -- bench.py prints the backend it used
        backend = os.environ.get("FRCNN_DIST_BACKEND") or ("nccl" if use_cuda else "gloo")
    if use_cuda:
        if backend == "gloo" and local_rank >= torch.cuda.device_count():
            local_rank %= torch.cuda.device_count()
        torch.cuda.set_device(local_rank)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "23456")       # the reference's fixed port (utils/__init__.py:16)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
        dist.barrier()
    device = torch.device("cuda", local_rank) if use_cuda else torch.device("cpu")
    return rank, local_rank, world, device


def shutdown():
    """Tear the process group down (quiet exit under torchrun); no-op for a single process."""
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def shard_indices(n_items, rank, world):
    """DistributedSampler-style partition (new_datasets/build.py:72): rank r takes r, r+W, r+2W, ..."""
    return list(range(rank, n_items, world))


def wrap_ddp(model, device, bucket_cap_mb=100):
    """models/build.py:8-14: DDP, find_unused_parameters=False.  No-op for a single process."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return model
    from torch.nn.parallel import DistributedDataParallel as DDP
    ids = [device.index] if device.type == "cuda" else None
    # broadcast_buffers=False: the only buffers of the two mirrors are the FROZEN batch-norm statistics of the ResNet-50-FPN backbone,
    # identical on every rank by construction; broadcasting them in every forward costs a collective per step and, being an in-place
    # copy, would invalidate the cached scale / shift of every FrozenBatchNorm2d (new_model.py) each iteration.
    return DDP(model, device_ids=ids, find_unused_parameters=False, bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True,
               broadcast_buffers=False)


def ddp_report(net):
    """What DDP's reducer was built over, from its own logging record: the number of parameter tensors it hooked (each
    parameter ONCE -- the VGG mirror registers `classifier` twice, as FRCNN.classifier and fast_rcnn_head.classifier, like the
    reference, models/model.py:282,298), their bytes, the bucket cap and the bucket sizes (initial assignment; DDP re-buckets
    in gradient-ready order after the first backward and reports that as rebuilt_bucket_sizes).  None for an unwrapped model."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    if not isinstance(net, DDP):
        return None
    d = net._get_ddp_logging_data()

    def sizes(key):
        v = d.get(key)
        return [int(x) for x in str(v).replace(",", " ").split()] if v not in (None, "") else None
    unique = {id(p): p for p in net.module.parameters() if p.requires_grad}
    return {"num_parameter_tensors": int(d.get("num_parameter_tensors", -1)), "total_parameter_size_bytes": int(d.get("total_parameter_size_bytes", -1)),
            "unique_trainable_parameters": len(unique), "unique_trainable_bytes": int(sum(p.numel() * p.element_size() for p in unique.values())),
            "registered_names_with_aliases": len(list(net.module.named_parameters(remove_duplicate=False))),
            "bucket_cap_bytes": int(d.get("bucket_cap_bytes", -1)), "bucket_sizes": sizes("bucket_sizes"),
            "rebuilt_bucket_sizes": sizes("rebuilt_bucket_sizes"), "gradient_as_bucket_view": bool(d.get("gradient_as_bucket_view", 0)),
            "find_unused_parameters": bool(d.get("find_unused_parameters", 0))}


def max_over_ranks(value, device):
    """MAX of a python float over all ranks (bench.py's timing rule)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return float(value)
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def gather_over_ranks(value, device):
    """The python float of every rank, as a list indexed by rank (bench.py prints per-rank step times)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return [float(value)]
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    out = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [float(o.item()) for o in out]


def sum_over_ranks(value, device):
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return float(value)
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


def barrier():
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()


class FrameSlot(object):
    """The one resident frame a captured training step reads: static device tensors at fixed addresses, refilled before every replay.

        x [1, 3, H, W] f32 | boxes [cap, 4] f32 | labels [cap] i64 | n_gt int32[1] | empty int32[1]

    The number of ground-truth boxes is DATA here (n_gt), not a shape: `model(slot.x, slot.boxes, slot.labels, n_gt=slot.n_gt,
    empty=slot.empty)` hands the target makers the whole fixed-capacity lists and they read the count on the device (ops.rpn_targets /
    ops.head_targets), so ONE captured graph set trains on any stream of frames -- straight from the device input stage
    (MosaicResult / CropResult / DeviceMultiScaleStage: boxes, labels, count), without the count.item() that slicing would need:

        slot = FrameSlot((H, W), cap, device)
        opt = DeviceSGD(params, ..., guard=slot.empty)          # a frame without boxes makes the captured update a no-op
        gs = GraphStep(model, opt, lambda f: loss_of(model(slot.x, slot.boxes, slot.labels, n_gt=slot.n_gt, empty=slot.empty)), 1, device,
                       **model.graph_stages()).capture()
        for i, (x, boxes, labels, count) in enumerate(stream):
            slot.load(x, boxes, labels, count)
            gs.step(i)

    `empty` is written by the head target maker at every step (1: the frame had no live box -- the reference raises there; the step's
    loss is NaN and, with guard=slot.empty, nothing is updated; 0 otherwise), never by load().  A count above the capacity cannot be
    refused without reading it: the first `cap` rows are used and _lib.HT_ERR_GT_COUNT lands in the model's sticky status word.

    One slot -- and one graph set -- serves ONE input shape.  A recipe with several padded shapes (the multi-scale stage) needs a slot
    and a GraphStep per distinct shape; choosing between them is the caller's (a shape-bucketing cache is not part of this class)."""

    def __init__(self, image_hw, gt_capacity, device):
        try:
            H, W = (int(v) for v in image_hw)
        except (TypeError, ValueError):
            raise ValueError("FrameSlot: image_hw must be (H, W), got %r" % (image_hw,))
        if H <= 0 or W <= 0:
            raise ValueError("FrameSlot: image_hw must be positive, got %r" % (image_hw,))
        if isinstance(gt_capacity, bool) or not isinstance(gt_capacity, int) or not 1 <= gt_capacity <= 4096:
            raise ValueError("FrameSlot: gt_capacity must be an int in [1, 4096] (the target makers' limit), got %r" % (gt_capacity,))
        self.device = torch.device(device)
        self.capacity = gt_capacity
        self.x = torch.zeros(1, 3, H, W, dtype=torch.float32, device=self.device)
        self.boxes = torch.zeros(gt_capacity, 4, dtype=torch.float32, device=self.device)
        self.labels = torch.zeros(gt_capacity, dtype=torch.int64, device=self.device)
        self.n_gt = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.empty = torch.zeros(1, dtype=torch.int32, device=self.device)

    def load(self, x, boxes, labels, count=None):
        """Stream-ordered copies into the static tensors; nothing is read back.  boxes [r, 4] / labels [r] with r <= capacity (rows
        r .. capacity are cleared); count: a device tensor of one element, a Python int, or None (= r).  Whatever the host knows is
        checked here (ValueError); a device count is checked by the kernels (see the class)."""
        if not torch.is_tensor(x) or tuple(x.shape[-3:]) != tuple(self.x.shape[1:]) or x.numel() != self.x.numel():
            raise ValueError("FrameSlot.load: x must be [1, 3, %d, %d] (one slot serves one input shape), got %s"
                             % (self.x.shape[2], self.x.shape[3], tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        if not torch.is_tensor(boxes) or boxes.dim() != 2 or boxes.shape[1] != 4:
            raise ValueError("FrameSlot.load: boxes must be [r, 4]")
        r = boxes.shape[0]
        if r > self.capacity:
            raise ValueError("FrameSlot.load: %d boxes, the slot holds %d" % (r, self.capacity))
        if not torch.is_tensor(labels) or labels.numel() != r:
            raise ValueError("FrameSlot.load: %d boxes need %d labels" % (r, r))
        if count is None:
            count = r
        if torch.is_tensor(count):
            if count.numel() != 1 or count.dtype.is_floating_point or count.dtype == torch.bool:
                raise ValueError("FrameSlot.load: count must be ONE integer")
        else:
            if isinstance(count, bool) or not isinstance(count, int):
                raise ValueError("FrameSlot.load: count must be a device tensor or a Python int, got %r" % (count,))
            if not 0 <= count <= r:
                raise ValueError("FrameSlot.load: count %d outside [0, %d rows]" % (count, r))
        with torch.no_grad():
            self.x.copy_(x.reshape(self.x.shape), non_blocking=True)
            self.boxes[:r].copy_(boxes, non_blocking=True)
            self.labels[:r].copy_(labels.reshape(-1), non_blocking=True)
            if r < self.capacity:
                self.boxes[r:].zero_()
                self.labels[r:].zero_()
            if torch.is_tensor(count):
                self.n_gt.copy_(count.reshape(1), non_blocking=True)
            else:
                self.n_gt.fill_(count)
        return self


class GraphStep(object):
    """The data-parallel training step of train.py:31-37 under models/build.py:8-14, submitted as HIP graphs instead of ~400 (VGG16) /
    ~2500 (ResNet-50-FPN) launches enqueued from Python, with the gradient all-reduce issued BETWEEN the replays (RCCL is not captured):

        replay A[f]   forward + loss + the backward of the head (FC layers behind the RoI pooling: 88 % of VGG16's gradient bytes),
                      those gradients written into one flat buffer
        all-reduce    of that buffer, asynchronously on the process group's own stream      -+  these two overlap: the
        replay B[f]   the rest of the backward (RoI pooling, RPN, backbone) -> a second flat buffer  -+  collective hides behind the trunk
        all-reduce    of the second buffer
        replay U      the optimizer step, reading p.grad = views into the two flat buffers

    A[f] / B[f] exist once per resident frame f (the SHAPE of a frame's ground-truth tensors is frozen into its graphs), U once.  To train on
    a stream of frames use n_frames = 1 and a forward_loss that reads a FrameSlot (above): the count of boxes is then device data.  The backward is cut at
    the output of `cut_module` (the RoI pooling) and at the RPN's predictions: A takes d loss / d {those tensors, head parameters} with
    torch.autograd.grad, B continues from them -- the same nodes the single backward() runs, each once, so the gradients are the
    ones DDP computes.  Like DDP's reducer the average is taken by scaling BEFORE the sum (here: the backward is seeded with 1 / world,
    exact for a power-of-two world, so the replicas match eager DDP bit for bit there; within rounding otherwise).
    Parameters are broadcast from rank 0 at construction, as DDP does.

    `forward_loss(f) -> (losses, pred)`: losses[0] is the scalar to minimise, pred the model's prediction tuple (pred[0], pred[1] = the
    RPN's class / box predictions).  `record(f, losses)` runs inside the capture right after the forward (copy what must survive the
    shared memory pool).  With graphs=False every piece runs eagerly (CPU tensors, gloo: the world-size-2 tests) through the same code.

    `accumulate=K` (default 1: nothing below applies, the code path is the one described above): gradient accumulation over windows of K
    steps, decided on the device (optim.GradAccumulator, csrc/grad_accum.hip), in the SAME graph set.  The backward is seeded with
    1 / (world * K) -- the gradient of loss / K, the torch idiom, and the mean over ranks as before; A and B run on every step and SUM
    into the flat buffers (a window's first step writes them, the later ones add: the bits of `grad.add_(g)`); the two all-reduces and U
    run only on the step that closes a window -- the host knows the phase, so the other steps issue no collective and replay no
    optimizer graph.  `frame_skip=`: a one-element int32 device tensor, typically the FrameSlot's `empty`: a frame for which it is
    non-zero is left out of its window -- its (NaN) gradients are not read, it contributes zero and the divisor stays K -- and a window
    whose frames were ALL left out updates nothing.  That last decision is the accumulator's `hold` word, which the optimizer must read as
    its guard.  The accumulator is made here, so the optimizer is HANDED OVER afterwards: construct with optimizer=None, build
    `DeviceSGD(..., guard=gs.accumulator.hold)`, then `gs.set_optimizer(opt)`, before capture().  A DeviceSGD with any other guard
    is refused.  (Another optimizer class does not read hold: it also steps after an all-empty window, on the zeros that window's first
    step wrote.)  At world > 1 the closing step also all-reduces hold with MIN, so every rank takes the same
    decision: step if any rank had a live frame; a rank whose window was empty contributes zeros.  The window state is not checkpointed: a
    resumed run starts a new window (reset_window()).  Both are this project's definitions -- the reference has no accumulation and raises
    on a frame without boxes (docs/PARITY.md).  K > 1 needs a HIP device."""

    def __init__(self, model, optimizer, forward_loss, n_frames, device, cut_module=None, late_modules=(), record=None, graphs=True,
                 accumulate=1, frame_skip=None):
        self.model, self.opt, self.forward_loss, self.n, self.device = model, optimizer, forward_loss, n_frames, device
        self.record = record
        self.graphs = bool(graphs) and device.type == "cuda"
        self.world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        self.accumulator, self.accumulate = None, 1
        if type(accumulate) is not int or accumulate != 1 or frame_skip is not None:      # the default takes no step into the new code
            self._init_accumulator(accumulate, frame_skip, device)
        params = [p for p in model.parameters() if p.requires_grad]                       # parameters() lists an aliased module's tensors once
        late_ids = {id(p) for m in late_modules for p in m.parameters() if p.requires_grad} if cut_module is not None else set()
        self.late = [p for p in params if id(p) in late_ids]
        self.early = [p for p in params if id(p) not in late_ids]
        self.cut_module = cut_module if self.late else None
        if self.world > 1:
            with torch.no_grad():
                for p in params:
                    dist.broadcast(p.data, 0)
                for b in model.buffers():
                    dist.broadcast(b.data, 0)
        self.flat, self.views = [], {}
        for group in (self.late, self.early):
            if not group:
                self.flat.append(None)
                continue
            assert all(p.dtype == group[0].dtype for p in group), "one dtype per flat buffer"
            buf = torch.zeros(sum(p.numel() for p in group), dtype=group[0].dtype, device=device)
            off = 0
            for p in group:
                self.views[id(p)] = buf[off:off + p.numel()].view_as(p)
                off += p.numel()
            self.flat.append(buf)
        for p in params:
            p.grad = self.views[id(p)]                                                    # for good: the optimizer graph reads these addresses
        self.seed = torch.full((), 1.0 / (self.world * self.accumulate), dtype=torch.float32, device=device)
        self._cut = []
        self.gA, self.gB, self.gU = [], [], None
        self.comm_bytes = [0 if b is None else b.numel() * b.element_size() for b in self.flat]
        if self.accumulator is not None and optimizer is not None:
            self._check_guard(optimizer)

    # ---- accumulation over a window of K steps (accumulate > 1)
    def _init_accumulator(self, accumulate, frame_skip, device):
        from .optim import GradAccumulator
        if isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1:
            raise ValueError("GraphStep: accumulate must be an int >= 1, got %r" % (accumulate,))
        if accumulate == 1:
            raise ValueError("GraphStep: frame_skip= is read by the accumulation only (accumulate > 1); with accumulate=1 a frame is "
                             "left out by the optimizer's guard")
        if torch.device(device).type != "cuda":
            raise ValueError("GraphStep: accumulate=%d needs a HIP device, got %s (the accumulation has no CPU fallback)" % (accumulate, device))
        self.accumulator, self.accumulate = GradAccumulator(accumulate, device, frame_skip=frame_skip), accumulate

    def _check_guard(self, optimizer):
        from .optim import DeviceSGD
        if isinstance(optimizer, DeviceSGD):
            g = optimizer.guard
            if g is None or g.data_ptr() != self.accumulator.hold.data_ptr():
                raise ValueError("GraphStep: with accumulate > 1 a DeviceSGD must be built with guard=<this GraphStep>.accumulator.hold (the "
                                 "word that keeps the update a no-op until a window with a live frame has closed)")

    def set_optimizer(self, optimizer):
        """For an optimizer that could only be built after this object (guard=self.accumulator.hold).  Before capture()."""
        if self.gU is not None:
            raise RuntimeError("GraphStep: the optimizer's graph is captured already")
        if self.accumulator is not None:
            self._check_guard(optimizer)
        self.opt = optimizer
        return self

    def reset_window(self):
        """The next step opens a window (device state and host mirror); outside graphs.  A no-op with accumulate=1."""
        if self.accumulator is not None:
            self.accumulator.reset_window()

    # ---- the pieces (eager or under capture)
    def _stage_a(self, f):
        h = None
        if self.cut_module is not None:
            del self._cut[:]
            h = self.cut_module.register_forward_hook(lambda mod, i, o: self._cut.append(o))
        try:
            losses, pred = self.forward_loss(f)
        finally:
            if h is not None:
                h.remove()
        if self.record is not None:
            self.record(f, losses)
        total = losses[0]
        seed = self.seed.to(total.dtype)
        if self.cut_module is None:
            grads = torch.autograd.grad([total], self.early, [seed], allow_unused=True)
            self._store(self.early, grads)
            if self.accumulator is not None:
                self.accumulator.advance()
            return None
        cuts = [t for t in list(self._cut) + [pred[0], pred[1]] if torch.is_tensor(t) and t.requires_grad]
        del self._cut[:]
        grads = torch.autograd.grad([total], cuts + self.late, [seed], retain_graph=True, allow_unused=True)
        self._store(self.late, grads[len(cuts):])
        live = [(t, g) for t, g in zip(cuts, grads[:len(cuts)]) if g is not None]
        return [t for t, _ in live], [g for _, g in live]

    def _stage_b(self, carry):
        roots, seeds = carry
        grads = torch.autograd.grad(roots, self.early, seeds, allow_unused=True)
        self._store(self.early, grads)
        if self.accumulator is not None:
            self.accumulator.advance()                  # once per step, behind the last _store: both stores saw the same phase

    def _store(self, params, grads):
        if any(g is None for g in grads):
            # torch's optimizers skip a parameter whose .grad is None (no weight decay, no momentum); a captured optimizer step cannot, so --
            # like DDP with find_unused_parameters=False (models/build.py:12) -- every trainable parameter must take part in the loss
            raise RuntimeError("GraphStep: %d trainable parameter(s) received no gradient" % sum(g is None for g in grads))
        if not params:
            return
        if self.accumulator is not None:                # write, add or leave out: decided on the device (a strided gradient is packed first, in the graph)
            self.accumulator.accumulate([self.views[id(p)] for p in params], [g if g.is_contiguous() else g.contiguous() for g in grads])
            return
        torch._foreach_copy_([self.views[id(p)] for p in params], list(grads))

    def _reduce(self, k):
        if self.world > 1 and self.flat[k] is not None:
            return dist.all_reduce(self.flat[k], op=dist.ReduceOp.SUM, async_op=True)
        return None

    def _reduce_hold(self):
        if self.world > 1:
            return dist.all_reduce(self.accumulator.hold, op=dist.ReduceOp.MIN, async_op=True)
        return None

    # ---- capture
    def capture(self, warm=1):
        """Eager warm-up passes on a side stream (lazy initialisation, optimizer state), then the graphs.  The warm-up steps UPDATE the
        weights; callers that need the initial weights (tests) restore them in place afterwards."""
        if not self.graphs:
            return self
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warm * self.accumulate):     # whole windows: the optimizer steps, the phase is back at 0
                for f in range(self.n):
                    self._eager(f)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # torch.cuda.graph no longer collects garbage before a capture (torch >= 2.9, unless torch.compiler.config.force_cudagraph_gc).  A
        # dead Python cycle that holds graphs or device memory -- an earlier GraphStep whose forward_loss closure refers back to its owner --
        # would otherwise be destroyed by whichever automatic collection comes next, possibly in the middle of a capture below, where
        # destroying a graph is not permitted and aborts the process.  Collect now, while nothing is capturing.
        gc.collect()
        pool = None
        for f in range(self.n):
            ga = torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga, pool=pool):
                carry = self._stage_a(f)
            pool = ga.pool()
            gb = None
            if carry is not None:
                gb = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gb, pool=pool):
                    self._stage_b(carry)
            del carry
            self.gA.append(ga)
            self.gB.append(gb)
        self.gU = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.gU, pool=pool):
            self.opt.step()
        self.sync_state()
        if self.accumulator is not None:
            self.accumulator.reset_window()
            self.accumulator.reset_stats()
        return self

    def sync_state(self):
        """Rank 0's parameters, buffers and optimizer state (momentum) to every rank, in place: whatever ran before (warm-up passes on each
        rank's own frames) the replicas are identical from here on."""
        if self.world == 1:
            return
        with torch.no_grad():
            ts = [p.data for p in self.late + self.early] + [b.data for b in self.model.buffers()]
            for p in self.late + self.early:
                ts += [v for _, v in sorted(self.opt.state.get(p, {}).items()) if torch.is_tensor(v)]
            for t in ts:
                dist.broadcast(t, 0)

    def _eager(self, f):
        if self.accumulator is not None:
            return self._eager_window(f)
        carry = self._stage_a(f)
        w0 = self._reduce(0)
        if carry is not None:
            self._stage_b(carry)
        w1 = self._reduce(1)
        for w in (w0, w1):
            if w is not None:
                w.wait()
        self.opt.step()

    def _eager_window(self, f):
        closing = self.accumulator.closing              # read before stage A / B: their advance() moves the mirror
        carry = self._stage_a(f)
        w0 = self._reduce(0) if closing else None
        if carry is not None:
            self._stage_b(carry)
        if closing:
            self._close_window(w0)
            self.opt.step()

    def _close_window(self, w0):
        for w in (w0, self._reduce(1), self._reduce_hold()):
            if w is not None:
                w.wait()

    def _step_window(self, f):
        """accumulate > 1: A and B on every step; the collectives and U only when the window closes."""
        closing = self.accumulator.closing
        self.gA[f].replay()
        w0 = self._reduce(0) if closing else None
        if self.gB[f] is not None:
            self.gB[f].replay()
        self.accumulator.tick()                         # the replayed advance() moved the device's phase
        if closing:
            self._close_window(w0)
            self.gU.replay()

    def step(self, i):
        f = i % self.n
        if not self.graphs:
            return self._eager(f)
        if self.accumulator is not None:
            return self._step_window(f)
        self.gA[f].replay()
        w0 = self._reduce(0)                            # on the process group's stream, behind what the replay enqueued
        if self.gB[f] is not None:
            self.gB[f].replay()
        w1 = self._reduce(1)
        for w in (w0, w1):
            if w is not None:
                w.wait()                                # the current stream waits for the collective; the host does not
        self.gU.replay()

    def report(self):
        return {"submission": "HIP graphs: A (forward + loss + head backward) | all-reduce | B (trunk backward) | all-reduce | optimizer" if self.graphs else "eager pieces",
                "world": self.world, "head_gradient_bytes": self.comm_bytes[0], "trunk_gradient_bytes": self.comm_bytes[1],
                "parameter_tensors": len(self.late) + len(self.early), "graphs": (len(self.gA) + sum(g is not None for g in self.gB) + 1) if self.graphs else 0,
                "accumulate": self.accumulate}
