"""Numpy restatement of csrc/grad_accum.hip (include/frcnn_hip.h: frcnn_grad_accumulate, frcnn_grad_accum_advance): fp32 adds in frame
order, one rounding each; the phase / frame_skip table; the advance rule.  The state is the block's seven words as a dict."""
import numpy as np

KEYS = ("window", "phase", "live", "hold", "windows", "frames", "dropped")
CHUNK = 8192


def new_state(window):
    s = dict.fromkeys(KEYS, 0)
    s["window"] = int(window)
    return s


def words(state):
    """The first seven int32 words of the block."""
    return [int(state[k]) for k in KEYS]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def accumulate(accs, srcs, state, frame_skip=0):
    """In place on the float32 arrays `accs`.  Where the kernel reads nothing, nothing is read here: a source is only touched when it is
    used, an accumulator only read when it is added to."""
    p, w = state["phase"], state["window"]
    if p < 0 or p >= w:
        return
    for a, s in zip(accs, srcs):
        assert a.dtype == np.float32 and a.shape == np.shape(s)
        if p == 0:
            a[...] = np.float32(0.0) if frame_skip != 0 else np.asarray(s, np.float32)
        elif frame_skip == 0:
            a[...] = a + np.asarray(s, np.float32)                          # float32 + float32: rounded once


def advance(state, frame_skip=0):
    p, w = state["phase"], state["window"]
    if p < 0 or p >= w:
        return state
    state["frames"] += 1
    state["dropped"] += int(frame_skip != 0)
    state["live"] += int(frame_skip == 0)
    if p + 1 == w:
        state["hold"] = int(state["live"] == 0)
        state["windows"] += 1
        state["phase"] = 0
        state["live"] = 0
    else:
        state["hold"] = 1
        state["phase"] = p + 1
    return state
