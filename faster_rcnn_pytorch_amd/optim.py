"""DeviceSGD: the reference's optimizer (main.py:58-61: torch.optim.SGD(lr, momentum, weight_decay); stepped at train.py:35-37) as ONE
library launch (csrc/sgd.hip) whose hyper-parameters live in device memory.

Why: a torch optimizer built with a Python-float lr passes the lr to its kernels as a launch constant, so a captured graph
(parallel.GraphStep, torch.cuda.graph) keeps the lr it was captured with whatever a scheduler does afterwards.  Here the kernel reads
(lr, momentum, weight_decay) per parameter group from a device block at run time; `param_groups[i]['lr']` stays a Python float that
any torch scheduler can change, and `push_hyper()` -- a stream-ordered write OUTSIDE the graph -- carries a change to the device.

The update rule is torch.optim.SGD's (dampening 0, no Nesterov, maximize=False), bit for bit against torch on the CPU
(tests/golden/sgd.npz, docs/PARITY.md).  Momentum tensors are allocated once, at construction, and never move: load_state_dict copies
INTO them.  Whether a tensor has had its first update is device data too (one int32 "born" word per tensor), so a graph captured before
any step is right from step 0 on, and a step skipped by the guard word leaves everything as it was.

Gradient clipping and the non-finite skip (csrc/grad_norm.hip) are device data as well.  With `max_grad_norm` and / or `skip_nonfinite`
two more launches in front of the update measure the global L2 norm of all trainable gradients (a binary64 sum in a fixed, documented
order: include/frcnn_hip.h) and count their non-finite elements; a clip coefficient -- torch.nn.utils.clip_grad_norm_'s
max_norm / (norm + 1e-6) clamped to 1 -- and a skip word land in a 64-byte state block, and the update multiplies the coefficient in as
it reads the gradient: no extra pass over the gradients, `p.grad` is NOT scaled in place, no host synchronisation, capturable, four
launches whatever the tensors are.  `max_grad_norm` is a Python float that `push_hyper()` carries to the device like the lr.  With both
options off nothing changes: the same two launches and no further allocation.

GradAccumulator (csrc/grad_accum.hip) sums the gradients of a window of K frames in front of ONE update -- write, add or leave a frame out,
decided on the device -- and its `hold` word is the guard that keeps the update off until a window with a live frame has closed.

WeightEMA (csrc/ema.hip) keeps an exponential moving average of the trainable weights in device memory: fused into DeviceSGD's update
kernel (`DeviceSGD(..., ema=)`: the kernel holds the new weight in registers when it stores it), gated by the same skip word as the step,
and exchanged with the live weights IN PLACE by a kernel, so that graphs captured on the parameters evaluate the averaged weights.

There is no fallback: anything the kernel does not cover (dampening, Nesterov, maximize, non-fp32, sparse or non-contiguous tensors or
gradients, a trainable parameter without a gradient, CPU tensors) is refused with an exception."""
import contextlib
import ctypes as C
import math
import struct

import torch

from . import _lib

GROUP_KEYS = ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "foreach", "differentiable", "fused")


def group_defaults(lr=1e-3, momentum=0, weight_decay=0, dampening=0, nesterov=False, maximize=False):
    """The per-group keys of torch.optim.SGD, in its order (a state dict of one loads into the other)."""
    return dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize,
                foreach=None, differentiable=False, fused=None)


def _check_group(g):
    if g["dampening"] != 0:
        raise ValueError("DeviceSGD: dampening != 0 is not supported (the reference uses 0, main.py:58-61)")
    if g["nesterov"]:
        raise ValueError("DeviceSGD: nesterov=True is not supported")
    if g["maximize"]:
        raise ValueError("DeviceSGD: maximize=True is not supported")
    if g.get("differentiable"):
        raise ValueError("DeviceSGD: differentiable=True is not supported")
    for k in ("lr", "momentum", "weight_decay"):
        v = g[k]
        if torch.is_tensor(v):
            raise ValueError("DeviceSGD: %s must be a Python number (the device block is written by push_hyper()), got a tensor" % k)
        if not float(v) >= 0.0:
            raise ValueError("DeviceSGD: invalid %s: %r" % (k, v))


def _check_max_grad_norm(v):
    if torch.is_tensor(v):
        raise ValueError("DeviceSGD: max_grad_norm must be a Python number (the device block is written by push_hyper()), got a tensor")
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or not v > 0:
        raise ValueError("DeviceSGD: invalid max_grad_norm: %r (a number > 0)" % (v,))
    return float(v)


# the state block of csrc/grad_norm.hip (frcnn_grad_norm_state, include/frcnn_hip.h): byte offsets, and the whole block for struct.unpack
GN_STATE_BYTES, GN_OFF_MAX_NORM, GN_OFF_FLAGS, GN_OFF_NORM, GN_OFF_COEF, GN_OFF_SKIP = 64, 0, 4, 16, 20, 24
GN_OFF_NONFINITE = 28
GN_STATE_FORMAT = "<fIdffiiii24x"
GN_CLIP, GN_SKIP_NONFINITE = 1, 2


def _check_dense(t, what, device=None, who="DeviceSGD", role="the optimizer"):
    if not torch.is_tensor(t) or t.layout != torch.strided or t.is_sparse:
        raise TypeError("%s: %s is not a dense strided tensor" % (who, what))
    if t.device.type != "cuda":
        raise RuntimeError("%s: %s is on %s: %s runs only on a HIP device (no CPU fallback)" % (who, what, t.device, role))
    if device is not None and t.device != device:
        raise RuntimeError("%s: %s is on %s, %s's tensors are on %s" % (who, what, t.device, role, device))
    if t.dtype != torch.float32:
        raise TypeError("%s: %s is %s: fp32 only" % (who, what, t.dtype))
    if not t.is_contiguous():
        raise TypeError("%s: %s is not contiguous (dense tensors only)" % (who, what))


# the state block of csrc/grad_accum.hip (frcnn_grad_accum_state, include/frcnn_hip.h): byte offsets, and the whole block for struct.unpack
GA_STATE_BYTES, GA_OFF_WINDOW, GA_OFF_PHASE, GA_OFF_LIVE, GA_OFF_HOLD, GA_OFF_WINDOWS = 64, 0, 4, 8, 12, 16
GA_STATE_FORMAT = "<iiiiiii36x"
GA_STATE_KEYS = ("window", "phase", "live", "hold", "windows", "frames", "dropped")


class GradAccumulator(object):
    """GradAccumulator(window, device, frame_skip=None): gradient accumulation over a window of `window` frames whose state lives in
    device memory (csrc/grad_accum.hip), so that ONE captured graph serves every micro-step of every window.

        acc = GradAccumulator(K, device, frame_skip=slot.empty)
        opt = DeviceSGD(params, ..., guard=acc.hold)          # p.grad are the tensors `accs` below
        per frame:  acc.accumulate(accs, grads)               # one call per group of tensors; all calls of a frame see the same phase
                    acc.advance()                             # once per frame, behind the last accumulate
                    opt.step()                                # may be attempted after EVERY frame: hold keeps it a no-op until a window closes

    A window's first frame WRITES the accumulators (they are not read: nothing has to be zeroed between windows), every later frame adds,
    one rounding per element -- the bits of torch's `grad.add_(g)`.  `frame_skip`: a one-element int32 device tensor (typically a
    FrameSlot's `empty`); while it is non-zero the frame is left out: its gradients are not read (they may be NaN), it contributes zero, and
    the divisor of the mean stays `window` (the caller seeds its backward with 1 / window).  A window whose frames were all left out
    closes with hold == 1: the optimizer does not step.  These are this project's definitions: the reference has no accumulation and
    raises on a frame without boxes (docs/PARITY.md).

    The host keeps a mirror of the phase (`closing`): advance() moves both when it runs eagerly.  Under capture it only records the
    launch -- nothing runs, so neither moves; whoever replays a graph that holds an advance() calls tick() once per replay.  The window
    state is not checkpointed: a resumed run starts a new window.  There is no CPU fallback."""

    def __init__(self, window, device, frame_skip=None):
        if isinstance(window, bool) or not isinstance(window, int) or window < 1:
            raise ValueError("GradAccumulator: window must be an int >= 1, got %r" % (window,))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GradAccumulator: device %s: the accumulation runs only on a HIP device (no CPU fallback)" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if frame_skip is not None:
            if not torch.is_tensor(frame_skip) or frame_skip.dtype != torch.int32 or frame_skip.numel() != 1 or frame_skip.device != self.device:
                raise TypeError("GradAccumulator: frame_skip must be a one-element int32 tensor on %s" % self.device)
        self.window, self.frame_skip = window, frame_skip
        with torch.no_grad():
            self._state = torch.zeros(GA_STATE_BYTES, dtype=torch.uint8, device=self.device)      # one address for good
            self._state[GA_OFF_WINDOW:GA_OFF_WINDOW + 4].view(torch.int32).fill_(window)
        self.hold = self._state[GA_OFF_HOLD:GA_OFF_HOLD + 4].view(torch.int32)
        self._phase = 0

    @property
    def closing(self):
        """Host bool: the next advance() closes a window."""
        return self._phase == self.window - 1

    def _pointers(self):
        skip = C.c_void_p(self.frame_skip.data_ptr()) if self.frame_skip is not None else None
        return C.c_void_p(self._state.data_ptr()), skip, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def accumulate(self, accs, grads):
        """One frcnn_grad_accumulate call: accs[i] = grads[i], or += grads[i], or nothing -- the table in the class docstring, decided on
        the device.  Dense contiguous fp32 tensors on this device, of equal shapes; anything else is refused."""
        accs, grads = list(accs), list(grads)
        if len(accs) != len(grads):
            raise ValueError("GradAccumulator: %d accumulators, %d gradients" % (len(accs), len(grads)))
        if not accs:
            return
        for k, (a, g) in enumerate(zip(accs, grads)):
            _check_dense(a, "accumulator %d" % k, self.device, "GradAccumulator", "the accumulation")
            _check_dense(g, "gradient %d" % k, self.device, "GradAccumulator", "the accumulation")
            if a.shape != g.shape:
                raise RuntimeError("GradAccumulator: gradient %d has shape %s, its accumulator %s" % (k, tuple(g.shape), tuple(a.shape)))
        n = len(accs)
        vp = C.c_void_p * n
        state, skip, stream = self._pointers()
        spare = self._state.data_ptr()                                    # an empty tensor has no address; its row is legal but may not be NULL
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.frcnn_grad_accumulate(n, vp(*[g.data_ptr() or spare for g in grads]), vp(*[a.data_ptr() or spare for a in accs]),
                                                      (C.c_int64 * n)(*[a.numel() for a in accs]), state, skip, stream), "frcnn_grad_accumulate")

    def tick(self):
        """The host mirror alone: once per replay of a graph that holds an advance()."""
        self._phase = (self._phase + 1) % self.window

    def advance(self):
        """Once per frame, behind its last accumulate(): frcnn_grad_accum_advance.  Run eagerly it moves the device state and the host
        mirror; under capture it records the launch and moves neither (see tick())."""
        state, skip, stream = self._pointers()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.frcnn_grad_accum_advance(state, skip, stream), "frcnn_grad_accum_advance")
        if not torch.cuda.is_current_stream_capturing():
            self.tick()

    def _outside_graphs(self, what):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradAccumulator: %s writes the state block from the host side and the stream is capturing: call it outside graphs" % what)

    def reset_window(self):
        """Phase and live count back to 0, on the device (stream-ordered, no synchronisation) and in the host mirror: the next frame opens
        a window.  What the accumulators hold is overwritten by that frame.  Outside graphs only."""
        self._outside_graphs("reset_window()")
        with torch.no_grad():
            self._state[GA_OFF_PHASE:GA_OFF_LIVE + 4].zero_()
        self._phase = 0

    def reset_stats(self):
        """The running counters (windows, frames, dropped) back to 0, e.g. after the warm-up passes of a capture.  Outside graphs only."""
        self._outside_graphs("reset_stats()")
        with torch.no_grad():
            self._state[GA_OFF_WINDOWS:GA_OFF_WINDOWS + 12].zero_()

    def stats(self):
        """The state block as a dict: window, phase, live, hold, windows, frames, dropped.  A device read-back: synchronises."""
        return dict(zip(GA_STATE_KEYS, struct.unpack(GA_STATE_FORMAT, bytes(self._state.cpu().numpy()))))


# the state block of csrc/ema.hip (frcnn_ema_state, include/frcnn_hip.h): the whole block for struct.pack / unpack
EMA_STATE_BYTES, EMA_STATE_FORMAT, EMA_WARMUP = 64, "<dqfIiii28x", 1
EMA_STATE_KEYS = ("decay", "num_updates", "w", "flags", "swapped", "skipped", "refused")


def ema_weight(decay, warmup, n):
    """The weight of update number n (n updates applied so far) in binary64, as csrc/ema.hip computes it on the device:
    decay_t = min(decay, (1 + n) / (10 + n)) under warm-up, else decay; w = 1 - decay_t.  The caller narrows it to float32."""
    return 1.0 - (min(decay, (1 + n) / (10 + n)) if warmup else decay)


def _build_table(builder, table, *rows):
    """One table build for prepare(): `builder` (frcnn_sgd_table_build_host or frcnn_ema_table_build_host) fills a pinned host block from
    `rows`, its leading arguments, and the block is uploaded into the device tensor `table` asynchronously.  Returns n_chunks."""
    host = torch.empty(table.numel(), dtype=torch.uint8).pin_memory()     # a fresh staging block per build: the copy below is asynchronous
    n_chunks = C.c_int32(0)
    _lib.check(getattr(_lib.lib, builder)(*rows, C.c_void_p(host.data_ptr()), table.numel(), C.byref(n_chunks)), builder)
    table.copy_(host, non_blocking=True)
    return int(n_chunks.value)


def _trainable(params):
    """Tensors or torch-style parameter groups -> the trainable parameters in DeviceSGD's row order."""
    out = []
    for item in params:
        for p in (item["params"] if isinstance(item, dict) else (item,)):
            if torch.is_tensor(p) and p.requires_grad:
                out.append(p)
    return out


class WeightEMA(object):
    """WeightEMA(params, decay=0.9998, warmup=True, guard=None, shadow=None): an exponential moving average of the trainable parameters,
    kept and updated in device memory (csrc/ema.hip), for evaluating and checkpointing.  The reference evaluates the raw weights and keeps
    no average: defined by this project, pinned to torch -- one update is torch._foreach_lerp_([e], [p], w) on the CPU bit for bit, which is
    what torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)) runs (tests/golden/ema.npz, docs/PARITY.md).

        ema = WeightEMA(params, decay=0.9998)
        opt = DeviceSGD(params, ..., ema=ema)       # the average rides in the update kernel and reads the step's skip word
        gs = GraphStep(model, opt, ...); gs.capture()
        ema.reset()                                 # capture()'s warm-up steps moved the weights AND the average
        ... train ...
        with ema.applied():                         # live <-> averaged, in place, by a kernel: every captured graph stays valid
            evaluate(model)
        save_checkpoint(path, epoch, model, opt, sched, ema=ema)

    `params`: tensors or parameter groups; the trainable ones (requires_grad) are averaged, in DeviceSGD's row order.  Frozen parameters and
    buffers are NOT averaged: in both mirrors the buffers are the frozen norms' statistics, which never change.  `decay`: a Python float,
    0 <= decay < 1, fixed here.  `warmup`: the weight of update n (n updates applied so far) is 1 - min(decay, (1 + n) / (10 + n)), so the
    average follows the weights closely at first; computed on the device, so replays follow it.  `guard`: a one-element int32 device tensor
    read by update() (a fused step reads the optimizer's skip word instead).  `shadow`: a list of caller tensors to average into (dense
    contiguous fp32, the parameters' shapes, overlapping nothing); by default one contiguous tensor per parameter is allocated.  Either way
    the shadows start as copies of the parameters and never move: load_state_dict copies INTO them.

    A step that is skipped -- the accumulator's hold, a FrameSlot's empty, a non-finite gradient -- is decided on the device; the average
    reads the same word, does not move and counts it (`skipped`).  Between swap() and swap() the parameters hold the averaged weights:
    an update() or a fused step then changes NOTHING, parameters included, and is counted (`refused`).  With GraphStep(accumulate=K) the
    average moves once per closed live window; under data parallelism every rank applies identical updates.  There is no CPU fallback;
    a non-fp32, sparse or non-contiguous parameter is refused, and so is a list without a trainable parameter."""

    def __init__(self, params, decay=0.9998, warmup=True, guard=None, shadow=None):
        if torch.is_tensor(decay) or isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
            raise ValueError("WeightEMA: invalid decay: %r (a Python number, 0 <= decay < 1)" % (decay,))
        self._decay, self.warmup = float(decay), bool(warmup)
        self._params = _trainable(params)
        if not self._params:
            raise ValueError("WeightEMA: no trainable parameter")
        self.device = self._params[0].device
        for k, p in enumerate(self._params):
            _check_dense(p, "parameter %d" % k, self.device if k else None, "WeightEMA", "the weight average")
        if guard is not None:
            if not torch.is_tensor(guard) or guard.dtype != torch.int32 or guard.numel() != 1 or guard.device != self.device:
                raise TypeError("WeightEMA: guard must be a one-element int32 tensor on %s" % self.device)
        self.guard = guard
        n = len(self._params)
        with torch.no_grad():
            if shadow is None:
                shadow = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in self._params]
            else:
                shadow = list(shadow)
                if len(shadow) != n:
                    raise ValueError("WeightEMA: %d shadow tensors for %d trainable parameters" % (len(shadow), n))
                for k, (e, p) in enumerate(zip(shadow, self._params)):
                    _check_dense(e, "shadow %d" % k, self.device, "WeightEMA", "the weight average")
                    if e.shape != p.shape:
                        raise RuntimeError("WeightEMA: shadow %d has shape %s, its parameter %s" % (k, tuple(e.shape), tuple(p.shape)))
                    if e.requires_grad:
                        raise RuntimeError("WeightEMA: shadow %d requires grad" % k)
            self.shadow = shadow                                              # allocated once; the kernels and every graph hold these addresses
            self._state = torch.zeros(EMA_STATE_BYTES, dtype=torch.uint8, device=self.device)
        self._numel = (C.c_int64 * n)(*[p.numel() for p in self._params])
        self._table_bytes = int(_lib.lib.frcnn_ema_table_bytes(n, self._numel))
        if self._table_bytes == 0:
            raise _lib.FrcnnError("WeightEMA: frcnn_ema_table_bytes refuses %d tensors of these sizes" % n)
        with torch.no_grad():
            self._table = torch.empty(self._table_bytes, dtype=torch.uint8, device=self.device)   # one address for good
        self._n_chunks, self._key = 0, None
        self.reset()

    @property
    def decay(self):
        return self._decay

    @decay.setter
    def decay(self, value):
        raise AttributeError("WeightEMA: decay is fixed at construction (the device block holds it; a decay that changes later is not built)")

    # ---- the state block and the table
    def _outside_graphs(self, what):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightEMA: %s writes the state block from the host side and the stream is capturing: call it outside graphs" % what)

    def _write_state(self, n):
        """decay, flags, num_updates = n and the weight for n; swapped and the counters zero.  Stream-ordered."""
        blob = struct.pack(EMA_STATE_FORMAT, self._decay, int(n), ema_weight(self._decay, self.warmup, int(n)), EMA_WARMUP if self.warmup else 0, 0, 0, 0)
        with torch.no_grad():
            self._state.copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))

    def prepare(self):
        """Builds and uploads the table for the current parameter addresses (a no-op when they have not moved).  update(), swap() and a
        fused step call it; call it yourself before capturing a graph that no eager call preceded."""
        key = tuple(p.data_ptr() for p in self._params) + tuple(e.data_ptr() for e in self.shadow)
        if key == self._key:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightEMA: a parameter address changed and the stream is capturing: call prepare() before the capture")
        n = len(self._params)
        vp = C.c_void_p * n
        spare = self._state.data_ptr()                                    # an empty tensor has no address; its row is legal but may not be NULL
        self._n_chunks = _build_table("frcnn_ema_table_build_host", self._table, n, vp(*[p.data_ptr() or spare for p in self._params]),
                                      vp(*[e.data_ptr() or spare for e in self.shadow]), self._numel)
        self._key = key

    def _head(self):
        return C.c_void_p(self._table.data_ptr()), self._table_bytes, len(self._params), self._n_chunks

    def fused_arguments(self):
        """(table, table bytes, state) for frcnn_sgd_step_ema: DeviceSGD.launch()."""
        self.prepare()
        return C.c_void_p(self._table.data_ptr()), self._table_bytes, C.c_void_p(self._state.data_ptr())

    # ---- launches
    def update(self):
        """The stand-alone update behind ANY optimizer's step: frcnn_ema_update, two launches, no host synchronisation, capturable.  With
        DeviceSGD(ema=) do not call it: the step already moved the average."""
        self.prepare()
        guard = C.c_void_p(self.guard.data_ptr()) if self.guard is not None else None
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib.frcnn_ema_update(*self._head(), C.c_void_p(self._state.data_ptr()), guard, stream), "frcnn_ema_update")

    def swap(self):
        """Live and averaged weights exchanged element for element IN PLACE (frcnn_ema_swap: one launch, no host synchronisation,
        capturable); no data_ptr() changes.  Two swaps are the identity."""
        self.prepare()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib.frcnn_ema_swap(*self._head(), C.c_void_p(self._state.data_ptr()), stream), "frcnn_ema_swap")

    @contextlib.contextmanager
    def applied(self):
        """with ema.applied(): the parameters hold the averaged weights inside the block (swap in, swap out)."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    @torch.no_grad()
    def copy_to(self):
        """Copies the shadow tensors into the parameters (the live weights are lost; the average stays)."""
        for p, e in zip(self._params, self.shadow):
            p.copy_(e)

    @torch.no_grad()
    def reset(self):
        """The average becomes a copy of what the parameters hold now; num_updates = 0, the weight for n = 0, swapped and the counters
        cleared.  Call it after GraphStep.capture(), whose warm-up steps move the average on each rank's own frames.  Outside graphs only."""
        self._outside_graphs("reset()")
        for p, e in zip(self._params, self.shadow):
            e.copy_(p)
        self._write_state(0)

    def stats(self):
        """The state block as a dict: decay, num_updates, w, warmup, swapped, skipped, refused.  A device read-back: synchronises."""
        d = dict(zip(EMA_STATE_KEYS, struct.unpack(EMA_STATE_FORMAT, bytes(self._state.cpu().numpy()))))
        d["warmup"] = bool(d.pop("flags") & EMA_WARMUP)
        return d

    # ---- checkpoints
    @torch.no_grad()
    def averaged_state_dict(self, model):
        """model.state_dict() with the averaged tensor (a copy) in place of every trainable parameter this object covers; frozen parameters
        and buffers as the model holds them.  Call it outside applied()."""
        by_id = dict((id(p), e) for p, e in zip(self._params, self.shadow))
        out = model.state_dict()
        for name, p in model.named_parameters(remove_duplicate=False):
            if id(p) in by_id and name in out:
                out[name] = by_id[id(p)].detach().clone()
        return out

    def state_dict(self):
        """decay, warmup, num_updates (a device read-back: synchronises) and the shadow tensors themselves, in row order."""
        return {"decay": self._decay, "warmup": self.warmup, "num_updates": self.stats()["num_updates"], "shadow": list(self.shadow)}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Copies the saved shadows INTO the existing tensors (no address changes) and sets num_updates and its weight; swapped and the
        counters are cleared.  decay and warmup are fixed at construction: a state dict that disagrees is refused.  Outside graphs only."""
        self._outside_graphs("load_state_dict()")
        if float(state_dict["decay"]) != self._decay or bool(state_dict["warmup"]) != self.warmup:
            raise ValueError("WeightEMA: the state dict was written with decay %r, warmup %r; this average has decay %r, warmup %r (fixed at construction)"
                             % (state_dict["decay"], state_dict["warmup"], self._decay, self.warmup))
        saved, n = list(state_dict["shadow"]), int(state_dict["num_updates"])
        if len(saved) != len(self.shadow):
            raise ValueError("WeightEMA: the state dict holds %d shadow tensors, this average %d" % (len(saved), len(self.shadow)))
        if n < 0:
            raise ValueError("WeightEMA: invalid num_updates: %r" % (n,))
        for k, (e, v) in enumerate(zip(self.shadow, saved)):
            if tuple(v.shape) != tuple(e.shape):
                raise ValueError("WeightEMA: saved shadow %d has shape %s, the parameter %s" % (k, tuple(v.shape), tuple(e.shape)))
        for e, v in zip(self.shadow, saved):
            e.copy_(v.to(device=self.device, dtype=torch.float32))
        self._write_state(n)


class DeviceSGD(torch.optim.Optimizer):
    """DeviceSGD(params, lr, momentum=0, weight_decay=0, guard=None, max_grad_norm=None, skip_nonfinite=False, ema=None, tensor_stats=None,
    after_step=None).  `guard`: a device int32
    tensor of one element; while it is non-zero a step changes nothing (parameters, momentum, born words).  Parameters with
    requires_grad=False take no part.

    `max_grad_norm`: a Python float > 0; the gradients enter the update multiplied by min(1, max_grad_norm / (norm + 1e-6)), norm the global
    L2 norm of all trainable gradients (norm_type 2 only).  The attribute may be changed later; push_hyper() (step() calls it) carries the
    new value to the device, outside graphs.  `skip_nonfinite`: a step whose gradients hold an inf or a NaN changes nothing and is counted.
    WHETHER the two are on is fixed here, because the launch sequence differs.  grad_stats() reads the last step's norm, coefficient,
    skip word and the counters back; grad_norm_tensor is the norm as a device scalar.

    The state dict stays torch.optim.SGD's, key for key: max_grad_norm and the counters (steps, skipped_steps) are NOT checkpointed --
    pass max_grad_norm to the constructor again on resume; the counters restart at zero.

    `ema`: a WeightEMA over exactly this optimizer's trainable parameters, in its row order; the average then rides in the update kernel
    (frcnn_sgd_step_ema: the update, the born launch, the average's bookkeeping), reads the step's skip word, and while the averaged
    weights are swapped in the whole step changes nothing.  The average has its own state dict.  With ema=None nothing changes: the same
    two or four launches and no further allocation.

    `tensor_stats`: True, or a dict of telemetry.TensorStats' keyword arguments (names, every): the optimizer builds a TensorStats over
    its own table (`opt.tensor_stats`) and launch() measures in front of frcnn_grad_norm and the update -- three more launches, gated
    by no skip word.  `after_step`: a callable run at the end of launch(), inside whatever graph captures the step -- a
    ScalarJournal.append of scalar_views() lands in GraphStep's optimizer graph.  With both None nothing changes: the same launches and
    no further allocation."""

    def __init__(self, params, lr=1e-3, momentum=0, weight_decay=0, dampening=0, nesterov=False, maximize=False, guard=None,
                 max_grad_norm=None, skip_nonfinite=False, norm_type=2.0, ema=None, tensor_stats=None, after_step=None):
        if torch.is_tensor(norm_type) or isinstance(norm_type, bool) or not isinstance(norm_type, (int, float)) or float(norm_type) != 2.0:
            raise ValueError("DeviceSGD: norm_type %r is not supported: the L2 norm only" % (norm_type,))
        self._clip, self._skip_nonfinite = max_grad_norm is not None, bool(skip_nonfinite)
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm) if self._clip else None
        super().__init__(params, group_defaults(lr, momentum, weight_decay, dampening, nesterov, maximize))
        self._rows = []                                                   # (parameter, group index), trainable parameters in state-dict order
        for gi, g in enumerate(self.param_groups):
            _check_group(g)
            for p in g["params"]:
                if p.requires_grad:
                    self._rows.append((p, gi))
        if not self._rows:
            raise ValueError("DeviceSGD: no trainable parameter")
        self.device = self._rows[0][0].device
        for k, (p, _) in enumerate(self._rows):
            _check_dense(p, "parameter %d" % k, self.device if k else None)
        if guard is not None:
            if not torch.is_tensor(guard) or guard.dtype != torch.int32 or guard.numel() != 1 or guard.device != self.device:
                raise TypeError("DeviceSGD: guard must be a one-element int32 tensor on %s" % self.device)
        self.guard = guard
        if ema is not None:
            if not isinstance(ema, WeightEMA):
                raise TypeError("DeviceSGD: ema must be a WeightEMA, got %s" % type(ema).__name__)
            if len(ema._params) != len(self._rows) or any(a is not b for a, (b, _) in zip(ema._params, self._rows)):
                raise ValueError("DeviceSGD: ema must cover exactly this optimizer's trainable parameters, in its row order (the fused kernel finds "
                                 "a tensor's shadow under its row number)")
        self.ema = ema
        n, G = len(self._rows), len(self.param_groups)
        with torch.no_grad():
            for p, _ in self._rows:                                       # allocated once; the kernel and every graph hold these addresses
                self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            self._born = torch.zeros(n, dtype=torch.int32, device=self.device)
            self._hyper = torch.zeros(G, 4, dtype=torch.float32, device=self.device)
        self._pushed = [None] * G                                         # what the device block holds, as Python floats
        self._numel = (C.c_int64 * n)(*[p.numel() for p, _ in self._rows])
        self._group = (C.c_int32 * n)(*[gi for _, gi in self._rows])
        self._table_bytes = int(_lib.lib.frcnn_sgd_table_bytes(n, self._numel))
        if self._table_bytes == 0:
            raise _lib.FrcnnError("DeviceSGD: frcnn_sgd_table_bytes refuses %d tensors of these sizes" % n)
        self._table = torch.empty(self._table_bytes, dtype=torch.uint8, device=self.device)     # one address for good
        self._n_chunks = 0
        self._key = None
        self._gn_state = self._gn_work = None                             # allocated by the first prepare() when clipping or skipping is on
        self._gn_work_bytes = 0
        self._pushed_max_norm = None
        if after_step is not None and not callable(after_step):
            raise TypeError("DeviceSGD: after_step must be callable, got %s" % type(after_step).__name__)
        self.after_step = after_step
        self.tensor_stats = None
        if tensor_stats is not None and tensor_stats is not False:
            if tensor_stats is not True and not isinstance(tensor_stats, dict):
                raise TypeError("DeviceSGD: tensor_stats must be True or a dict of TensorStats' keyword arguments (names, every), got %s"
                                % type(tensor_stats).__name__)
            from .telemetry import TensorStats
            self.tensor_stats = TensorStats(self, **(tensor_stats if isinstance(tensor_stats, dict) else {}))

    # ---- hyper-parameters
    def push_hyper(self):
        """Writes the (lr, momentum, weight_decay) that changed since the last call into the device block: one stream-ordered fill per
        changed value, no host synchronisation.  Never part of a graph: under capture a pending change is an error.  max_grad_norm travels
        the same way (into the state block, once prepare() has allocated it), and so does tensor_stats.every."""
        self._push_max_norm()
        if self.tensor_stats is not None:
            self.tensor_stats.push()
        for gi, g in enumerate(self.param_groups):
            _check_group(g)
            now = (float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]))
            old = self._pushed[gi]
            if old == now:
                continue
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceSGD: group %d's hyper-parameters changed and the stream is capturing: the device block is written "
                                   "outside graphs -- call push_hyper() before the capture and before each replay" % gi)
            with torch.no_grad():
                for k in range(3):
                    if old is None or old[k] != now[k]:
                        self._hyper[gi, k].fill_(now[k])
            self._pushed[gi] = now

    def _push_max_norm(self):
        if not self._clip:
            if self.max_grad_norm is not None:
                raise ValueError("DeviceSGD: max_grad_norm was None at construction: whether gradients are clipped is fixed there (the launch "
                                 "sequence differs)")
            return
        if self.max_grad_norm is None:
            raise ValueError("DeviceSGD: max_grad_norm cannot be switched off after construction (the launch sequence differs)")
        now = _check_max_grad_norm(self.max_grad_norm)
        if self._gn_state is None or now == self._pushed_max_norm:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DeviceSGD: max_grad_norm changed and the stream is capturing: the device block is written outside graphs -- "
                               "call push_hyper() before the capture and before each replay")
        with torch.no_grad():
            self._gn_state[GN_OFF_MAX_NORM:GN_OFF_MAX_NORM + 4].view(torch.float32).fill_(now)
        self._pushed_max_norm = now

    # ---- the table
    def _gradients(self):
        gs = []
        for k, (p, _) in enumerate(self._rows):
            if not p.requires_grad:
                raise RuntimeError("DeviceSGD: parameter %d was trainable at construction and is frozen now" % k)
            g = p.grad
            if g is None:
                raise RuntimeError("DeviceSGD: trainable parameter %d has no gradient (.grad is None): a captured step cannot skip a tensor" % k)
            _check_dense(g, "the gradient of parameter %d" % k, self.device)
            if g.shape != p.shape:
                raise RuntimeError("DeviceSGD: the gradient of parameter %d has shape %s, the parameter %s" % (k, tuple(g.shape), tuple(p.shape)))
            gs.append(g)
        return gs

    def prepare(self):
        """Builds and uploads the table for the current parameter / gradient addresses (a no-op when they have not moved).  step() calls it;
        call it yourself before capturing a graph that no eager step preceded."""
        if self.ema is not None:
            self.ema.prepare()
        gs = self._gradients()
        key = tuple(p.data_ptr() for p, _ in self._rows) + tuple(g.data_ptr() for g in gs)
        if key == self._key:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DeviceSGD: a parameter or gradient address changed and the stream is capturing: run one eager step (or "
                               "prepare()) on the final gradient tensors before the capture")
        n = len(self._rows)
        if (self._clip or self._skip_nonfinite) and self._gn_state is None:   # once; the kernels and every graph hold these addresses
            chunks = _lib.sgd_chunks(self._numel)
            self._gn_work_bytes = int(_lib.lib.frcnn_grad_norm_workspace_bytes(chunks))
            with torch.no_grad():
                self._gn_work = torch.empty(self._gn_work_bytes, dtype=torch.uint8, device=self.device)
                self._gn_state = torch.zeros(GN_STATE_BYTES, dtype=torch.uint8, device=self.device)
                self._gn_state[GN_OFF_FLAGS:GN_OFF_FLAGS + 4].view(torch.int32).fill_((GN_CLIP if self._clip else 0) |
                                                                                    (GN_SKIP_NONFINITE if self._skip_nonfinite else 0))
            self._push_max_norm()
        vp = C.c_void_p * n
        self._n_chunks = _build_table("frcnn_sgd_table_build_host", self._table, n, vp(*[p.data_ptr() for p, _ in self._rows]),
                                      vp(*[g.data_ptr() for g in gs]), vp(*[self.state[p]["momentum_buffer"].data_ptr() for p, _ in self._rows]),
                                      self._numel, self._group, len(self.param_groups))
        self._key = key

    def launch(self):
        """The library launches alone (what a graph records): no hyper-parameter write.  With tensor_stats its three launches come first
        (they run whatever the skip word says); after_step() runs behind the update, inside whatever graph captures the step."""
        self.prepare()
        if self.tensor_stats is not None:
            self.tensor_stats.push()                                      # a pending `every` under capture is an error, as a pending lr
            self.tensor_stats._launch()
        self._launch_update()
        if self.after_step is not None:
            self.after_step()

    def _launch_update(self):
        guard = C.c_void_p(self.guard.data_ptr()) if self.guard is not None else None
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        head = (C.c_void_p(self._table.data_ptr()), self._table_bytes, len(self._rows), self._n_chunks)
        tail = (C.c_void_p(self._hyper.data_ptr()), len(self.param_groups), C.c_void_p(self._born.data_ptr()))
        ema = self.ema.fused_arguments() if self.ema is not None else None
        if not (self._clip or self._skip_nonfinite):
            if ema is not None:
                _lib.check(_lib.lib.frcnn_sgd_step_ema(*head, *tail, guard, None, *ema, stream), "frcnn_sgd_step_ema")
            else:
                _lib.check(_lib.lib.frcnn_sgd_step(*head, *tail, guard, stream), "frcnn_sgd_step")
            return
        state = self._gn_state.data_ptr()                                 # the guard goes INTO the state block's skip word
        _lib.check(_lib.lib.frcnn_grad_norm(*head, C.c_void_p(state), guard, C.c_void_p(self._gn_work.data_ptr()), self._gn_work_bytes, stream),
                   "frcnn_grad_norm")
        skip = C.c_void_p(state + GN_OFF_SKIP)
        if ema is not None:
            _lib.check(_lib.lib.frcnn_sgd_step_ema(*head, *tail, skip, C.c_void_p(state + GN_OFF_COEF) if self._clip else None, *ema, stream),
                       "frcnn_sgd_step_ema")
        elif self._clip:
            _lib.check(_lib.lib.frcnn_sgd_step_scaled(*head, *tail, skip, C.c_void_p(state + GN_OFF_COEF), stream), "frcnn_sgd_step_scaled")
        else:
            _lib.check(_lib.lib.frcnn_sgd_step(*head, *tail, skip, stream), "frcnn_sgd_step")

    # ---- the gradient norm of the last step
    def _need_state(self):
        if not (self._clip or self._skip_nonfinite):
            raise RuntimeError("DeviceSGD: no gradient norm is measured: construct with max_grad_norm and / or skip_nonfinite=True")
        if self._gn_state is None:
            raise RuntimeError("DeviceSGD: the state block is allocated by the first prepare() / step()")

    @property
    def grad_norm_tensor(self):
        """The last measured global gradient norm: a 0-d float32 view of the state block on the device (no copy, no synchronisation) --
        for logging from inside a capture."""
        self._need_state()
        return self._gn_state[GN_OFF_NORM:GN_OFF_NORM + 4].view(torch.float32)[0]

    def scalar_views(self):
        """0-d device views (no copy, no synchronisation) of the update-level scalars, for a ScalarJournal appended from after_step:
        "lr/<group>" per parameter group (float32, from the hyper block) and, where a gradient norm is measured, "grad_norm", "clip_coef"
        (float32), "skip" and "nonfinite" (int32) of the state block (allocated by the first prepare())."""
        views = {"lr/%d" % gi: self._hyper[gi, 0] for gi in range(len(self.param_groups))}
        if self._clip or self._skip_nonfinite:
            self._need_state()
            f32 = lambda off: self._gn_state[off:off + 4].view(torch.float32)[0]          # noqa: E731
            i32 = lambda off: self._gn_state[off:off + 4].view(torch.int32)[0]            # noqa: E731
            views.update(grad_norm=f32(GN_OFF_NORM), clip_coef=f32(GN_OFF_COEF), skip=i32(GN_OFF_SKIP), nonfinite=i32(GN_OFF_NONFINITE))
        return views

    def grad_stats(self):
        """The state block after the last step, as a dict: norm, coef, skip, nonfinite, steps, skipped_steps, sumsq (and max_norm as the
        device holds it).  A device read-back: synchronises."""
        self._need_state()
        max_norm, _, sumsq, norm, coef, skip, nonfinite, steps, skipped = struct.unpack(GN_STATE_FORMAT, bytes(self._gn_state.cpu().numpy()))
        return dict(norm=norm, coef=coef, skip=skip, nonfinite=nonfinite, steps=steps, skipped_steps=skipped, sumsq=sumsq, max_norm=max_norm)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.push_hyper()
        with torch.cuda.device(self.device):
            self.launch()
        return loss

    def add_param_group(self, param_group):
        if getattr(self, "_table", None) is not None:
            raise RuntimeError("DeviceSGD: parameter groups are fixed at construction (the momentum tensors and the table are allocated there)")
        super().add_param_group(param_group)

    # ---- checkpoints: torch.optim.SGD's format
    def born(self):
        """The born words as a list of 0 / 1, one per trainable parameter (a device read-back: synchronises)."""
        return [int(v) for v in self._born.cpu().tolist()]

    def state_dict(self):
        born = dict(zip((id(p) for p, _ in self._rows), self.born()))
        state, groups, idx = {}, [], 0
        for g in self.param_groups:
            packed = {k: v for k, v in g.items() if k != "params"}
            packed["params"] = list(range(idx, idx + len(g["params"])))
            for i, p in zip(packed["params"], g["params"]):
                if born.get(id(p)):
                    state[i] = {"momentum_buffer": self.state[p]["momentum_buffer"]}
            idx += len(g["params"])
            groups.append(packed)
        return {"state": state, "param_groups": groups}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        if any(len(s["params"]) != len(g["params"]) for s, g in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        for s in saved:
            merged = group_defaults()
            merged.update({k: v for k, v in s.items() if k != "params"})
            _check_group(merged)
        by_index = {}
        for s, g in zip(saved, self.param_groups):
            for i, p in zip(s["params"], g["params"]):
                by_index[id(p)] = state_dict["state"].get(i, state_dict["state"].get(str(i)))
        born, copies = [], []
        for k, (p, _) in enumerate(self._rows):
            buf = (by_index.get(id(p)) or {}).get("momentum_buffer")
            if buf is not None:
                if tuple(buf.shape) != tuple(p.shape):
                    raise ValueError("DeviceSGD: the momentum of parameter %d has shape %s, the parameter %s" % (k, tuple(buf.shape), tuple(p.shape)))
                copies.append((self.state[p]["momentum_buffer"], buf))
            born.append(0 if buf is None else 1)
        for dst, src in copies:                                           # INTO the tensors allocated at construction: no address changes
            dst.copy_(src.to(device=self.device, dtype=torch.float32))
        self._born.copy_(torch.tensor(born, dtype=torch.int32))
        for s, g in zip(saved, self.param_groups):
            for k, v in s.items():
                if k != "params":
                    g[k] = v
        self.push_hyper()
