"""Device-side training telemetry (csrc/telemetry.hip): a record of a graph-replayed run that costs no host synchronisation and survives
capture.  The reference prints its five losses and the lr every vis_step steps (train.py:39-72) from host floats smoothed by SmoothedValue
(util/misc.py:27-86) -- one loss.item() per step.  Here the record stays on the device until somebody asks for it:

TensorStats   per-tensor statistics over a DeviceSGD's table: for every trainable tensor the L2 norms of gradient, weight and momentum
              (binary64 sums of squares in the fixed order include/frcnn_hip.h documents), max |g| and max |w|, the non-finite counts of
              g and w, and the name of the first tensor that holds an inf or a NaN.  Three launches whatever the tensors are, in front of
              the update (`DeviceSGD(..., tensor_stats=)`), capturable; `every=N` measures every Nth call, decided on the device, so one
              graph serves.  It runs whatever the optimizer's skip word says: the skipped step is the one whose culprit is wanted.
ScalarJournal one row of up to 64 device scalars per append into a ring, with running totals per column; `smoothed()` evaluates the
              reference's SmoothedValue expressions on the host from ONE copy.

Everything TensorStats reports is defined by this project; so are the journal's finite-only totals.  What is pinned to the reference:
for a column of finite fp32 values `sum` is the bits of SmoothedValue.total and smoothed() returns its median / avg / global_avg / max /
value (tests/golden/journal.npz, docs/PARITY.md).

Losses and update-level scalars are TWO journals: the losses exist once per frame (append them from `GraphStep(record=)`, which sees the
step's loss tensors inside the capture), lr / grad norm / clip coefficient / skip word once per update (append them from
`DeviceSGD(after_step=)`, which lands in GraphStep's optimizer graph).  Under accumulate=K there are K loss rows per update row.

There is no fallback: both objects run only on a HIP device."""
import ctypes as C
import struct

import numpy as np
import torch

from . import _lib

# frcnn_tensor_stats_row / frcnn_tensor_stats_state (include/frcnn_hip.h): sizes and byte offsets
TS_ROW_BYTES, TS_STATE_BYTES = 64, 64
TS_ROW_DTYPE = np.dtype([("g_sumsq", "<f8"), ("p_sumsq", "<f8"), ("m_sumsq", "<f8"), ("g_absmax", "<f4"), ("p_absmax", "<f4"),
                         ("g_nonfinite", "<i4"), ("p_nonfinite", "<i4"), ("m_read", "<i4"), ("reserved", "<i4", (5,))])
TS_STATE_FORMAT = "<iiiiii40x"
TS_STATE_KEYS = ("every", "tick", "measured_tick", "measures", "first_nonfinite_g", "first_nonfinite_p")
TS_OFF_EVERY = 0
# frcnn_journal_totals / frcnn_journal_state
JR_TOTALS_DTYPE = np.dtype([("sum", "<f8"), ("count", "<i8"), ("max", "<f8"), ("min", "<f8"), ("nonfinite", "<i8")])
JR_STATE_BYTES, JR_MAX_COLS = 64, 64
JR_DTYPES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3}
assert TS_ROW_DTYPE.itemsize == TS_ROW_BYTES and JR_TOTALS_DTYPE.itemsize == 40


def _check_every(v):
    if torch.is_tensor(v) or isinstance(v, bool) or not isinstance(v, int) or v < 1 or v > 2 ** 31 - 1:
        raise ValueError("TensorStats: every must be a Python int >= 1 (the device block is written by push()), got %r" % (v,))
    return v


def _cuda_device(device, who):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("%s: device %s: the telemetry runs only on a HIP device (no CPU fallback)" % (who, device))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class TensorStats(object):
    """TensorStats(optimizer, names=None, every=1): per-tensor statistics over `optimizer`'s table (a DeviceSGD), one row per trainable
    parameter in the optimizer's row order.  `names`: one string per row (default "0", "1", ...).  Rows, state block and workspace are
    allocated here, once, at addresses graphs can hold.

        stats = TensorStats(opt, names, every=50)       # or DeviceSGD(..., tensor_stats=dict(names=names, every=50)) -> opt.tensor_stats
        stats.measure()                                 # three launches; DeviceSGD.launch() makes them in front of the update
        r = stats.read()                                # ONE device-to-host copy (synchronises)
        r["tensors"]["backbone.conv1.weight"]["grad_norm"], r["first_nonfinite_g"], r["measured_tick"]

    `every` is a Python int that push() carries to the device by a stream-ordered fill OUTSIDE graphs (measure() calls it; under capture
    a pending change is an error, as DeviceSGD.push_hyper's).  Call k measures when k % every == 0, counted from construction; the rows
    keep the last measured values in between.  `rows_tensor` [n, 64] uint8 and `state_tensor` [64] uint8 are device views for use
    inside a capture."""

    def __init__(self, optimizer, names=None, every=1):
        from .optim import DeviceSGD
        if not isinstance(optimizer, DeviceSGD):
            raise TypeError("TensorStats: optimizer must be a DeviceSGD (its table is what the kernels walk), got %s" % type(optimizer).__name__)
        n = len(optimizer._rows)
        if names is None:
            names = [str(k) for k in range(n)]
        names = list(names)
        if len(names) != n or any(not isinstance(s, str) for s in names):
            raise ValueError("TensorStats: names must be %d strings, one per trainable parameter in the optimizer's row order" % n)
        if len(set(names)) != n:
            raise ValueError("TensorStats: names must be distinct")
        self.optimizer, self.names, self.every = optimizer, names, _check_every(every)
        self.device = optimizer.device
        self._n = n
        self._chunks = _lib.sgd_chunks(optimizer._numel)
        self._work_bytes = int(_lib.lib.frcnn_tensor_stats_workspace_bytes(n, self._chunks))
        if self._work_bytes == 0:
            raise _lib.FrcnnError("TensorStats: frcnn_tensor_stats_workspace_bytes refuses %d tensors in %d chunks" % (n, self._chunks))
        init = np.zeros(TS_STATE_BYTES + n * TS_ROW_BYTES, np.uint8)
        struct.pack_into(TS_STATE_FORMAT, init, 0, self.every, 0, -1, 0, -1, -1)
        self._init = torch.from_numpy(init)
        with torch.no_grad():
            self._block = torch.empty(init.size, dtype=torch.uint8, device=self.device)      # state | rows: one allocation, one copy to read
            self._block.copy_(self._init)
            self._work = torch.empty(self._work_bytes, dtype=torch.uint8, device=self.device)
        self._pushed_every = self.every

    @property
    def state_tensor(self):
        return self._block[:TS_STATE_BYTES]

    @property
    def rows_tensor(self):
        return self._block[TS_STATE_BYTES:].view(self._n, TS_ROW_BYTES)

    def push(self):
        """Carries a changed `every` to the device: one stream-ordered fill, no host synchronisation.  Never part of a graph."""
        now = _check_every(self.every)
        if now == self._pushed_every:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TensorStats: every changed and the stream is capturing: the device block is written outside graphs -- "
                               "call push() before the capture and before each replay")
        with torch.no_grad():
            self._block[TS_OFF_EVERY:TS_OFF_EVERY + 4].view(torch.int32).fill_(now)
        self._pushed_every = now

    def reset(self):
        """Rows zero, tick 0, nothing measured yet; `every` stays.  Outside graphs only."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TensorStats: reset() while the stream is capturing: the block is reset outside graphs")
        struct.pack_into("<i", self._init.numpy(), TS_OFF_EVERY, _check_every(self.every))
        with torch.no_grad():
            self._block.copy_(self._init)
        self._pushed_every = self.every

    def measure(self):
        """The three launches (what a graph records), on the optimizer's current table."""
        self.push()
        self.optimizer.prepare()
        self._launch()

    def _launch(self):
        opt = self.optimizer
        base = self._block.data_ptr()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib.frcnn_tensor_stats(
                C.c_void_p(opt._table.data_ptr()), opt._table_bytes, self._n, opt._n_chunks, C.c_void_p(opt._born.data_ptr()),
                C.c_void_p(base + TS_STATE_BYTES), C.c_void_p(base), C.c_void_p(self._work.data_ptr()), self._work_bytes, stream),
                "frcnn_tensor_stats")

    @staticmethod
    def decode(block, names):
        """bytes of state | rows -> the dict read() returns (host only)."""
        raw = bytes(block)
        out = dict(zip(TS_STATE_KEYS, struct.unpack(TS_STATE_FORMAT, raw[:TS_STATE_BYTES])))
        rows = np.frombuffer(raw[TS_STATE_BYTES:], TS_ROW_DTYPE)
        with np.errstate(all="ignore"):
            out["tensors"] = {
                name: dict(grad_norm=float(np.sqrt(r["g_sumsq"])), weight_norm=float(np.sqrt(r["p_sumsq"])), momentum_norm=float(np.sqrt(r["m_sumsq"])),
                           grad_absmax=float(r["g_absmax"]), weight_absmax=float(r["p_absmax"]), grad_nonfinite=int(r["g_nonfinite"]),
                           weight_nonfinite=int(r["p_nonfinite"]), momentum_read=int(r["m_read"]))
                for name, r in zip(names, rows)}
        for k in ("first_nonfinite_g", "first_nonfinite_p"):
            out[k + "_index"] = out[k]
            out[k] = names[out[k]] if 0 <= out[k] < len(names) else None
        return out

    def read(self):
        """One device-to-host copy (synchronises): {"tensors": {name: dict(grad_norm, weight_norm, momentum_norm, grad_absmax,
        weight_absmax, grad_nonfinite, weight_nonfinite, momentum_read)}, every, tick, measured_tick, measures, first_nonfinite_g,
        first_nonfinite_p (the tensor's NAME, or None) and the two row indices under ..._index}.  The norms are the square roots, in
        binary64, of the sums the device keeps."""
        return self.decode(self._block.cpu().numpy(), self.names)


class ScalarJournal(object):
    """ScalarJournal(names, capacity, device): a ring of the last `capacity` rows of len(names) <= 64 scalars, written on the device.

        losses = ScalarJournal(["loss", "rpn_cls", "rpn_reg", "roi_cls", "roi_reg"], capacity=100, device=dev)
        step = GraphStep(..., record=lambda out: losses.append([out[k] for k in keys]))      # one row per frame, inside the capture
        if i % vis_step == 0:
            print(losses.smoothed(window=20))                                                # ONE copy; median, avg, global_avg, max, value

    append(tensors, mark=None): one-element device tensors of float32 / float64 / int32 / int64 (anything else is refused here); every
    value is widened to binary64.  `mark`: a one-element int32 device tensor (a step counter) copied beside the row; 0 without one.  Per
    column the device keeps sum (sequential binary64, append order), count, max, min over the FINITE values and counts the others, which
    land in the ring as they are."""

    def __init__(self, names, capacity, device):
        names = list(names)
        if not 1 <= len(names) <= JR_MAX_COLS or any(not isinstance(s, str) for s in names) or len(set(names)) != len(names):
            raise ValueError("ScalarJournal: names must be 1 .. %d distinct strings, got %r" % (JR_MAX_COLS, names))
        if isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity <= 2 ** 31 - 1:
            raise ValueError("ScalarJournal: capacity must be an int >= 1, got %r" % (capacity,))
        self.device = _cuda_device(device, "ScalarJournal")
        self.names, self.capacity = names, capacity
        n = len(names)
        self._off_totals = JR_STATE_BYTES
        self._off_ring = self._off_totals + 40 * n                        # a multiple of 8
        self._off_marks = self._off_ring + 8 * capacity * n
        self._bytes = self._off_marks + 4 * capacity
        init = np.zeros(self._bytes, np.uint8)
        struct.pack_into("<qii", init, 0, 0, capacity, n)
        totals = init[self._off_totals:self._off_ring].view(JR_TOTALS_DTYPE)
        totals["max"], totals["min"] = -np.inf, np.inf
        self._init = torch.from_numpy(init)
        with torch.no_grad():
            self._block = torch.empty(self._bytes, dtype=torch.uint8, device=self.device)    # state | totals | ring | marks: one allocation, one copy to read
            self._block.copy_(self._init)

    def reset(self):
        """Empties ring, marks and totals.  Outside graphs only."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ScalarJournal: reset() while the stream is capturing: the journal is reset outside graphs")
        with torch.no_grad():
            self._block.copy_(self._init)

    def append(self, tensors, mark=None):
        """One launch of one wave on the current stream; capturable."""
        tensors = list(tensors)
        n = len(self.names)
        if len(tensors) != n:
            raise ValueError("ScalarJournal: %d values for %d columns" % (len(tensors), n))
        for name, t, dtypes, text in [(k, v, JR_DTYPES, "float32, float64, int32 and int64") for k, v in zip(self.names, tensors)] + \
                ([("mark", mark, (torch.int32,), "int32")] if mark is not None else []):
            if not torch.is_tensor(t) or t.layout != torch.strided:
                raise TypeError("ScalarJournal: %s is not a dense tensor (a Python number would be frozen into a graph)" % name)
            if t.device != self.device:
                raise RuntimeError("ScalarJournal: %s is on %s, the journal on %s (no CPU fallback)" % (name, t.device, self.device))
            if t.numel() != 1:
                raise ValueError("ScalarJournal: %s has %d elements: one-element tensors only" % (name, t.numel()))
            if t.dtype not in dtypes:
                raise TypeError("ScalarJournal: %s is %s: %s only" % (name, t.dtype, text))
        base = self._block.data_ptr()
        src = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
        codes = (C.c_int32 * n)(*[JR_DTYPES[t.dtype] for t in tensors])
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.lib.frcnn_journal_append(
                n, src, codes, self.capacity, C.c_void_p(base + self._off_ring), C.c_void_p(base + self._off_marks), C.c_void_p(base + self._off_totals),
                C.c_void_p(base), C.c_void_p(mark.data_ptr()) if mark is not None else None, stream), "frcnn_journal_append")

    def decode(self, block, last=None):
        """bytes of the block -> the dict read() returns (host only)."""
        raw = np.frombuffer(bytes(block), np.uint8)
        n, cap = len(self.names), self.capacity
        cursor = struct.unpack_from("<q", raw, 0)[0]
        totals = raw[self._off_totals:self._off_ring].view(JR_TOTALS_DTYPE)
        ring = raw[self._off_ring:self._off_marks].view(np.float64).reshape(cap, n)
        marks = raw[self._off_marks:].view(np.int32)
        have = min(cursor, cap) if last is None else min(cursor, cap, int(last))
        order = [(cursor - have + k) % cap for k in range(have)]           # append order, oldest first
        return dict(cursor=int(cursor), names=list(self.names), rows=ring[order].copy(), marks=marks[order].copy(),
                    totals={name: {k: (float(t[k]) if k in ("sum", "max", "min") else int(t[k])) for k in JR_TOTALS_DTYPE.names}
                            for name, t in zip(self.names, totals)})

    def read(self, last=None):
        """One device-to-host copy (synchronises): dict(cursor, names, rows [k, n] float64 in append order (the last min(cursor,
        capacity, last) rows), marks [k] int32, totals {name: dict(sum, count, max, min, nonfinite)})."""
        if last is not None and (isinstance(last, bool) or not isinstance(last, int) or last < 0):
            raise ValueError("ScalarJournal: last must be None or an int >= 0, got %r" % (last,))
        return self.decode(self._block.cpu().numpy(), last)

    def smoothed(self, window=20, data=None):
        """SmoothedValue (util/misc.py:27-86) per column over the last `window` rows of one read() (or of `data`, a dict read() returned):
        {name: dict(median, avg, global_avg, max, value, count)} with the reference's expressions -- torch.median of the window as the
        default float tensor, a float32 mean, total / count, max of the window, the last value.  A column without rows is left out."""
        if isinstance(window, bool) or not isinstance(window, int) or window < 1:
            raise ValueError("ScalarJournal: window must be an int >= 1, got %r" % (window,))
        data = self.read() if data is None else data
        return smoothed_from(data, window)


def smoothed_from(data, window=20):
    """The host half of ScalarJournal.smoothed: `data` is what read() returns."""
    out = {}
    rows = data["rows"][-window:] if len(data["rows"]) else data["rows"]
    for c, name in enumerate(data["names"]):
        dq = [float(v) for v in rows[:, c]]
        t = data["totals"][name]
        if not dq or t["count"] == 0:
            continue
        out[name] = dict(median=torch.tensor(dq).median().item(), avg=torch.tensor(dq, dtype=torch.float32).mean().item(),
                         global_avg=t["sum"] / t["count"], max=max(dq), value=dq[-1], count=t["count"])
    return out
