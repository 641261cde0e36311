"""Guard-band harness: run an op with every allocation between two poisoned guards and every scratch workspace at exactly the size
the op asked for, then say who wrote outside what.

    with guarded(0xFF) as g:
        x = g.place(x)                      # a test-made input, copied between guards of its own
        y = ops.some_op(x)                  # torch.empty & co. inside the op are served from arenas
        g.outputs(y=y)                      # declared outputs must live in an arena (checked by address)
    # on exit: synchronize, every guard byte still `fill`, control words zero, patched functions restored

An arena is one allocation `[guard | payload | guard]` of the ORIGINAL torch.empty: 256 KiB guards, the payload at the arena's
start + 256 KiB (so it keeps the 512-byte alignment torch's allocator gives) and of exactly the bytes asked for; the right guard starts
at the payload's last byte + 1.  Guards, the payloads of empty / empty_like and scratch are filled with the byte `fill`; zeros / full
keep their value; control workspaces are zero.  While the context is active
  * torch.empty, empty_like, zeros, zeros_like and full are replaced (device tensors only, unless guard_cpu=True);
  * ops._workspace / ops._ctrl_workspace and the name transforms.py imported (`transforms._workspace`) return a FRESH exact-size arena
    per call -- the package's grow-only 1 MiB floor and its "largest layer seen" control block are what hide a short size report;
    evaluation.py's per-evaluator cache (_RecordStore._workspace) is replaced too: one exact-size workspace per evaluator and (D, G), a
    control arena whose ticket and winner words are checked for zero (VOC) or scratch filled with `fill` (COCO);
  * ops._WS, _CTRL, _CTRL_IN_GRAPHS and _CONST are put back as they were on exit, so no cache entry points into an arena afterwards.
A control workspace that an op documents as read across calls is kept for the tags in keep_ctrl, or inside `with g.sharing_ctrl(tag)`
(one arena, as long as the size asked for stays the same).

What (a) the exit check cannot see -- a load from a guard, an element never stored -- shows when the same case runs under 0xFF and
under 0x00 and the two runs are compared: first_difference() names the output and the element.
"""
import contextlib
import sys

import torch

GUARD = 256 * 1024
_THIS = __file__.rsplit(".", 1)[0]

# tag -> byte ranges (begin, end) of the control workspace that the op documents as "left zero by every call" (include/frcnn_hip.h and
# the carve functions in csrc/): clipped to the workspace's size.
#   rpn_conv_f32 : two blocks of CF_MAX_TILES = 32768 ticket words in front of the transposed weights and slabs (rpn_conv_f32.hip cf_carve)
#   det_loss     : "its first word is the ticket ... that workgroup leaves the ticket zero"
#   rpn_targets  : the arrival counter and the last-workgroup ticket of RpnCtl (bytes 128 .. 1280), and the per-GT maxima: RPN_MAX_G = 4096
#                  lines of 64 bytes behind the control block and the 256-byte Philox snapshot (targets.hip carve_rpn)
#   eval         : the 64-byte ticket (eval.hip) for a workspace handed to ops.eval_update's own default; an evaluator's workspace also
#                  gets the winner words, whose extent depends on G (Guarded._evaluator_workspace)
CTRL_ZERO = {
    "rpn_conv_f32": ((0, 2 * 32768 * 4),),
    "det_loss": ((0, 4),),
    "rpn_targets": ((128, 1280), (1536, 1536 + 4096 * 64)),
    "eval": ((0, 64),),
}


class GuardError(AssertionError):
    pass


def _site():
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename.rsplit(".", 1)[0] == _THIS:
        f = f.f_back
    if f is None:
        return "?"
    named = f
    while named.f_back is not None and named.f_code.co_name.startswith("<"):          # a comprehension or lambda: name the function it stands in
        named = named.f_back
    return "%s:%d %s" % (f.f_code.co_filename.rsplit("/", 1)[-1], f.f_lineno, named.f_code.co_name)


class Arena(object):
    __slots__ = ("base", "nbytes", "kind", "site", "shape", "dtype", "tag", "tensor", "zero")

    def describe(self):
        what = self.kind if self.tag is None else "%s[%s]" % (self.kind, self.tag)
        return "%s %s %s (%d bytes) allocated at %s" % (what, tuple(self.shape), str(self.dtype).replace("torch.", ""), self.nbytes, self.site)

    def begin(self):
        return self.base.data_ptr() + GUARD

    def guards(self):
        return (("before", self.base[:GUARD]), ("after", self.base[GUARD + self.nbytes:]))


def _run(bad):
    """bool mask of touched bytes -> (index of the first, index of the last, how many are touched).  Two separate places touched in one
    guard are reported as one span first .. last with the number of touched bytes inside it."""
    idx = torch.nonzero(bad).reshape(-1)
    return int(idx[0]), int(idx[-1]), int(idx.numel())


class Guarded(object):
    def __init__(self, fill, guard_cpu=False, keep_ctrl=()):
        if fill not in (0x00, 0xFF):
            raise ValueError("fill is 0xFF or 0x00")
        self.fill = fill
        self.guard_cpu = guard_cpu
        self.keep_ctrl = tuple(keep_ctrl)
        self.arenas = []
        self._kept = {}
        self._declared = []
        self._orig = None

    # ---- arenas -------------------------------------------------------------------------------------------------------------
    def _arena(self, shape, dtype, device, kind, payload_fill, tag=None):
        o = self._orig
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        item = o["empty"]((), dtype=dtype).element_size()
        a = Arena()
        a.nbytes = numel * item
        a.base = o["empty"]((2 * GUARD + a.nbytes,), dtype=torch.uint8, device=device)
        a.base.fill_(self.fill)
        a.kind, a.site, a.shape, a.dtype, a.tag, a.zero = kind, _site(), shape, dtype, tag, None
        t = o["empty"]((0,), dtype=dtype, device=device)
        strides, st = [], 1
        for s in reversed(shape):
            strides.append(st)
            st *= max(s, 1)
        t.set_(a.base.untyped_storage(), GUARD // item, shape, tuple(reversed(strides)))
        assert t.data_ptr() == a.begin() or numel == 0
        if payload_fill is not None:
            t.fill_(payload_fill)
        a.tensor = t
        self.arenas.append(a)
        return t

    def _wants(self, device):
        device = torch.device(device) if device is not None else self._orig["empty"](0).device
        return device.type == "cuda" or (self.guard_cpu and device.type == "cpu")

    @staticmethod
    def _plain(kw):
        """Only dtype / device / requires_grad (and the default layout, memory format, pinning): anything else goes to torch itself."""
        for k, v in kw.items():
            if k in ("dtype", "device", "requires_grad"):
                continue
            if (k == "memory_format" and v in (torch.contiguous_format, torch.preserve_format)) or (k == "layout" and v == torch.strided) \
                    or (k == "pin_memory" and not v):
                continue
            return False
        return True

    @staticmethod
    def _size(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            return tuple(args[0])
        return tuple(args)

    def _make(self, name, payload_fill):
        orig = self._orig[name]

        def fn(*size, **kw):
            if not size and "size" in kw:
                kw = dict(kw)
                size = (kw.pop("size"),)
            if not self._plain(kw) or not self._wants(kw.get("device")):
                return orig(*size, **kw)
            try:
                shape = tuple(int(s) for s in self._size(size))
            except (TypeError, ValueError):
                return orig(*size, **kw)
            t = self._arena(shape, kw.get("dtype") or torch.get_default_dtype(), kw.get("device"), name, payload_fill)
            return t.requires_grad_() if kw.get("requires_grad") else t
        fn.__name__ = name
        return fn

    def _make_like(self, name, payload_fill):
        orig = self._orig[name]

        def fn(ref, **kw):
            dev = kw.get("device", ref.device)
            if not self._plain(kw) or not self._wants(dev) or ref.layout != torch.strided \
                    or (kw.get("memory_format", torch.preserve_format) == torch.preserve_format and not ref.is_contiguous()):
                return orig(ref, **kw)
            t = self._arena(ref.shape, kw.get("dtype") or ref.dtype, dev, name, payload_fill)
            return t.requires_grad_() if kw.get("requires_grad") else t
        fn.__name__ = name
        return fn

    def _make_full(self):
        orig = self._orig["full"]

        def fn(size, fill_value, **kw):
            if not self._plain(kw) or not self._wants(kw.get("device")) or isinstance(fill_value, torch.Tensor):
                return orig(size, fill_value, **kw)
            dtype = kw.get("dtype")
            if dtype is None:
                dtype = torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int) else torch.get_default_dtype()
            t = self._arena(self._size((size,)), dtype, kw.get("device"), "full", fill_value)
            return t.requires_grad_() if kw.get("requires_grad") else t
        return fn

    # ---- the package's scratch --------------------------------------------------------------------------------------------------
    def _scratch(self, device, nbytes):
        return self._arena((int(nbytes),), torch.uint8, device, "scratch", None)

    def _ctrl(self, device, tag, nbytes, zero=None, fresh=False):
        """zero: the byte ranges left zero, where they depend on the call (default: CTRL_ZERO[tag]); fresh: never a kept arena"""
        key = (tag, torch.device(device).index)
        if fresh:
            t = self._arena((int(nbytes),), torch.uint8, device, "ctrl", 0, tag=tag)
            self.arenas[-1].zero = zero
            return t
        if tag in self.keep_ctrl:
            t = self._kept.get(key)
            if t is not None:
                if t.numel() != int(nbytes):
                    raise GuardError("control workspace %r is kept across calls but was asked for at %d and then %d bytes" % (tag, t.numel(), int(nbytes)))
                return t
        t = self._arena((int(nbytes),), torch.uint8, device, "ctrl", 0, tag=tag)
        self.arenas[-1].zero = zero
        if tag in self.keep_ctrl:
            self._kept[key] = t
        return t

    def _evaluator_workspace(self):
        """evaluation._RecordStore._workspace keeps the update kernel's workspace per evaluator and (D, G) and allocates it with torch.zeros.
        Here it stays one workspace per evaluator and (D, G) -- the VOC kernel's contract is a DEDICATED block that is zero before the first
        call and left zero, so consecutive updates share it -- but it is a control arena ("eval": the 64-byte ticket and the winner words
        [EVAL_MAX_T][G] u64 at byte 256 must be zero on exit, csrc/eval.hip) for the VOC protocol, and scratch filled with `fill` for the COCO
        protocol, whose key segments may hold anything (csrc/coco_eval.hip)."""
        from faster_rcnn_pytorch_amd import _lib, evaluation
        guard = self

        def _workspace(ev, D, G):
            ws = ev._ws.get((D, G))
            if ws is None:
                nb = _lib.workspace_bytes(ev._OP[1], D, G)
                if nb == 0:
                    raise evaluation.FrcnnError("%s: detection capacity %d / ground-truth capacity %d outside the kernel's limits" % (ev._OP[0], D, G))
                if ev._OP[1] == _lib.OP_EVAL:
                    ws = guard._ctrl(ev.device, "eval", nb, zero=((0, 64), (256, 256 + evaluation.MAX_THRESHOLDS * int(G) * 8)), fresh=True)
                else:
                    ws = guard._scratch(ev.device, nb)
                ev._ws[(D, G)] = ws
            return ws
        return _workspace

    # ---- what a case calls --------------------------------------------------------------------------------------------------
    def place(self, tensor):
        """A copy of a test-made input between guards of its own (None stays None; grad requirement is kept)."""
        if tensor is None:
            return None
        src = tensor.detach()
        t = self._arena(src.shape, src.dtype, src.device, "place", None)
        t.copy_(src)
        return t.requires_grad_() if tensor.requires_grad else t

    def outputs(self, **named):
        """Declares the case's outputs: each must live inside an arena.  None values (an output not asked for) are skipped."""
        for name, t in named.items():
            if t is not None:
                self._declared.append((name, t))
        return named

    @contextlib.contextmanager
    def sharing_ctrl(self, tag):
        """Inside this block the calls that ask for control workspace `tag` get ONE arena (for calls documented to read what the call
        before them left there); before and after it every call gets a fresh one again."""
        self.keep_ctrl = self.keep_ctrl + (tag,)
        try:
            yield
        finally:
            self.keep_ctrl = tuple(t for t in self.keep_ctrl if t != tag)
            for key in [k for k in self._kept if k[0] == tag]:
                del self._kept[key]

    def expect_arenas(self, function, shapes):
        """For an op whose result torch derives from buffers the caller never sees (a gather, a product with a scalar): asserts that the
        allocations made in `function` of the package include arenas of these shapes, i.e. that the buffers the kernels write are guarded."""
        have = [a.shape for a in self.arenas if a.site.endswith(" " + function)]
        for shape in shapes:
            shape = tuple(int(v) for v in shape)
            if shape not in have:
                raise GuardError("no arena of shape %s was allocated in %s (arenas from there: %s): its buffers ran unguarded" % (shape, function, have))
            have.remove(shape)

    def arena_of(self, t):
        if t.numel() == 0:
            return next((a for a in self.arenas if a.tensor.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()), None)
        p, q = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        for a in self.arenas:
            if a.begin() <= p and q <= a.begin() + a.nbytes and a.base.device == t.device:
                return a
        return None

    # ---- enter / exit -------------------------------------------------------------------------------------------------------
    def __enter__(self):
        from faster_rcnn_pytorch_amd import ops, transforms
        from faster_rcnn_pytorch_amd import evaluation
        self._mods = (ops, transforms)
        self._orig_ev = (evaluation._RecordStore, evaluation._RecordStore._workspace)
        self._orig = {n: getattr(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like", "full")}
        self._orig_ws = (ops._workspace, ops._ctrl_workspace, transforms._workspace)
        self._caches = [(d, dict(d)) for d in (ops._WS, ops._CTRL, ops._CTRL_IN_GRAPHS, ops._CONST)]
        torch.empty = self._make("empty", None)
        torch.zeros = self._make("zeros", 0)
        torch.empty_like = self._make_like("empty_like", None)
        torch.zeros_like = self._make_like("zeros_like", 0)
        torch.full = self._make_full()
        ops._workspace = transforms._workspace = self._scratch
        ops._ctrl_workspace = self._ctrl
        evaluation._RecordStore._workspace = self._evaluator_workspace()
        return self

    def _restore(self):
        ops, transforms = self._mods
        for n, f in self._orig.items():
            setattr(torch, n, f)
        ops._workspace, ops._ctrl_workspace, transforms._workspace = self._orig_ws
        self._orig_ev[0]._workspace = self._orig_ev[1]
        for d, was in self._caches:
            d.clear()
            d.update(was)

    def __exit__(self, et, ev, tb):
        self._restore()
        if et is not None:
            return False
        self.check()
        return False

    def check(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        problems = []
        fill = self.fill
        flags = [torch.stack([(g != fill).any() for _, g in a.guards()]) for a in self.arenas]        # enqueue all, then read: one wait
        for a, hit in zip(self.arenas, [f.tolist() for f in flags]):
            for (side, g), h in zip(a.guards(), hit):
                if not h:
                    continue
                first, last, n = _run(g != fill)
                # offsets are relative to the payload: before = bytes in front of its first byte, after = bytes behind its last byte
                where = ("%d .. %d bytes before the start" % (GUARD - last, GUARD - first)) if side == "before" \
                    else ("%d .. %d bytes past the end" % (first, last))
                problems.append("guard %s the payload touched: %d bytes, %s, of %s" % (side, n, where, a.describe()))
        for a in self.arenas:
            if a.kind != "ctrl":
                continue
            for lo, hi in (a.zero if a.zero is not None else CTRL_ZERO.get(a.tag, ())):
                lo, hi = min(lo, a.nbytes), min(hi, a.nbytes)
                words = a.tensor[lo:hi]
                if hi > lo and bool((words != 0).any()):
                    first, last, n = _run(words != 0)
                    problems.append("control words not left zero: %d bytes in %d .. %d of %s" % (n, lo + first, lo + last, a.describe()))
        for name, t in self._declared:
            if self.arena_of(t) is None and (t.is_cuda or self.guard_cpu):
                problems.append("output %r %s %s does not live in an arena: allocated some other way, it ran unguarded"
                                % (name, tuple(t.shape), str(t.dtype).replace("torch.", "")))
        if problems:
            raise GuardError("\n".join(problems))


def guarded(fill, guard_cpu=False, keep_ctrl=()):
    """Context manager: see the module's docstring."""
    return Guarded(fill, guard_cpu=guard_cpu, keep_ctrl=keep_ctrl)


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.reshape(-1).view(torch.uint8).reshape(t.numel(), -1) if t.numel() else t.reshape(0, 1).view(torch.uint8)


def first_difference(a, b):
    """None when a and b hold the same bytes, else (flat element index, number of differing elements)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return (-1, -1)
    d = (_bits(a) != _bits(b.to(a.device))).any(dim=1)
    if not bool(d.any()):
        return None
    idx = torch.nonzero(d).reshape(-1)
    return int(idx[0]), int(idx.numel())


def assert_same_bits(name, a, b, what="the 0xFF and the 0x00 run"):
    """(b) of the guard tests: the defined part of an output is the same bytes whatever surrounds the operands and whatever the output
    and the scratch held before.  A difference is an element the op never wrote, or a value that depends on bytes outside the operands."""
    d = first_difference(a, b)
    if d is not None:
        i, n = d
        raise GuardError("output %r %s differs between %s in %d elements, first at flat element %d (%r vs %r): an element left "
                         "unwritten, or a result that depends on bytes outside the operands"
                         % (name, tuple(a.shape), what, n, i, a.reshape(-1)[i].item() if i >= 0 else a.shape, b.reshape(-1)[i].item() if i >= 0 else b.shape))


def run_both(case, **kw):
    """Runs `case(g)` under guarded(0xFF) and under guarded(0x00).  The case builds its inputs with g.place, calls the op and returns a
    dict of the DEFINED parts of its outputs; tensors in it are declared (so they must live in arenas), cloned out after the exit checks,
    and compared bit for bit between the two runs unless named in `only_reference` (an op not documented as bit-reproducible).
    `derived` names results that torch itself computes from the op's buffers (a gather, a product with a scalar): compared, but not
    expected to live in an arena -- the buffers they come from do, and are guarded.  A tuple of names, or a predicate on the name.
    Returns (outputs under 0xFF, outputs under 0x00)."""
    only_reference = tuple(kw.pop("only_reference", ()))
    derived = kw.pop("derived", ())
    is_derived = derived if callable(derived) else (lambda k: k in derived)
    res = []
    for fill in (0xFF, 0x00):
        with guarded(fill, **kw) as g:
            out = case(g)
            g.outputs(**{k: v for k, v in out.items() if isinstance(v, torch.Tensor) and not is_derived(k)})
        res.append({k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
    for k in res[0]:
        if isinstance(res[0][k], torch.Tensor) and k not in only_reference:
            assert_same_bits(k, res[0][k], res[1][k])
    return res[0], res[1]
