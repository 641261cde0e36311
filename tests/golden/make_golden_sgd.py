"""Writes tests/golden/sgd.npz: torch.optim.SGD (dampening 0, no Nesterov, maximize=False -- what main.py:58-61 constructs) run on the CPU.

Small cases keep their inputs; long ones keep a seed (tests/sgd_ref.py: seeded_inputs) and the sha256 of the inputs.  Of the results the
file keeps, per step, the sha256 of the bit patterns of all parameters and all momenta (NaN canonical, unborn momentum as zeros) and the
born flags; and the arrays after the last step for the cases that are small enough.  Run:  python tests/golden/make_golden_sgd.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sgd_ref  # noqa: E402

CHUNK = 8192                                     # csrc/sgd_dev.h: SGD_CHUNK
SWEEP1, SWEEP4 = 1024, 4096                      # csrc/multi_tensor_dev.h: the elements of one dword sweep and of one 16-byte sweep
LENS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257]
KEEP_INPUTS_BELOW = 4096
KEEP_FINAL_BELOW = 20000


def run_torch(lens, group, hyper, p0, g):
    """hyper [S, G, 3].  Returns per step: p [N], m [N] (zeros where there is no buffer), born [T]."""
    S, G = hyper.shape[:2]
    off = np.concatenate([[0], np.cumsum(lens)])
    params = [torch.nn.Parameter(torch.from_numpy(p0[off[t]:off[t + 1]].copy())) for t in range(len(lens))]
    groups = [{"params": [p for t, p in enumerate(params) if group[t] == gi], "lr": float(hyper[0, gi, 0]), "momentum": float(hyper[0, gi, 1]),
               "weight_decay": float(hyper[0, gi, 2])} for gi in range(G)]
    opt = torch.optim.SGD(groups, lr=1.0)
    assert all(pg["dampening"] == 0 and not pg["nesterov"] and not pg["maximize"] for pg in opt.param_groups)
    out = []
    for s in range(S):
        for gi, pg in enumerate(opt.param_groups):
            pg["lr"], pg["momentum"], pg["weight_decay"] = (float(v) for v in hyper[s, gi])
        for t, p in enumerate(params):
            p.grad = torch.from_numpy(g[s, off[t]:off[t + 1]].copy())
        opt.step()
        pm, born = np.zeros(len(p0), np.float32), np.zeros(len(lens), np.int32)
        for t, p in enumerate(params):
            buf = opt.state[p].get("momentum_buffer")
            if buf is not None:
                pm[off[t]:off[t + 1]], born[t] = buf.numpy(), 1
        out.append((np.concatenate([p.detach().numpy().ravel() for p in params]).astype(np.float32), pm, born))
    return out


def hyper_table(steps, rows):
    """rows: per group a list of (lr, mu, wd) per step, or one triple for every step."""
    return np.array([[r[s] if isinstance(r, list) else r for r in rows] for s in range(steps)], np.float64)


def main():
    torch.set_flush_denormal(False)
    rs = np.random.RandomState(20240607)
    kinds = {}
    cases = []

    def rand(n, scale):
        return (rs.standard_normal(n) * scale).astype(np.float32)

    # A: every short length, five steps, the lr changed between steps 2 and 3, the special gradient values
    lens = list(LENS)
    N = sum(lens)
    p0, g = rand(N, 0.1), np.stack([rand(N, 0.02) for _ in range(5)])
    g[0, 70:74] = 0.0; g[1, 70:72] = 0.0; g[2, 10] = -0.0; g[0, 11] = -0.0; g[3, 200:204] = -0.0      # exact zeros and -0.0
    g[1, 300] = np.nan                                                                                   # one NaN gradient element
    p0[400:408] = np.float32(3e-38); g[:, 400:408] = np.float32(1e-37)                                   # lr * m lands below 2^-126
    lr = [2e-3, 2e-3, 2e-4, 2e-4, 2e-4]
    cases.append(("lengths_five_steps", lens, [0] * len(lens), hyper_table(5, [[(v, 0.9, 5e-4) for v in lr]]), p0, g))
    kinds["short lengths"] = len(set(lens) & set(LENS))
    kinds["five steps"] = 5
    kinds["lr changed between steps 2 and 3"] = int(lr[1] != lr[2])
    kinds["zero gradients"] = int((g == 0).sum() - (np.signbit(g) & (g == 0)).sum())
    kinds["-0.0 gradients"] = int((np.signbit(g) & (g == 0)).sum())
    kinds["NaN gradients"] = int(np.isnan(g).sum())

    # B: weight decay 0 with infinite parameters
    lens = [5, 64, 9]
    N = sum(lens)
    p0, g = rand(N, 0.1), np.stack([rand(N, 0.02) for _ in range(3)])
    p0[2], p0[20], p0[70] = np.inf, -np.inf, np.inf
    cases.append(("wd0_inf_parameter", lens, [0] * 3, hyper_table(3, [(1e-2, 0.9, 0.0)]), p0, g))
    kinds["wd = 0 with an infinite parameter"] = int(np.isinf(p0).sum())

    # C: no momentum
    lens = [7, 65]
    N = sum(lens)
    cases.append(("momentum_zero", lens, [0, 0], hyper_table(3, [(1e-2, 0.0, 5e-4)]), rand(N, 0.1), np.stack([rand(N, 0.02) for _ in range(3)])))
    kinds["momentum = 0"] = 1

    # D: two groups with their own lr / weight decay (and momentum)
    lens = [5, 64, 257, 3, 65]
    N = sum(lens)
    cases.append(("two_groups", lens, [0, 1, 0, 1, 1], hyper_table(5, [(2e-3, 0.9, 5e-4), (1e-2, 0.8, 0.0)]), rand(N, 0.1),
                  np.stack([rand(N, 0.02) for _ in range(5)])))
    kinds["two groups"] = 2

    # E: one length on either side of the kernel's chunk, and the chunk itself      F: 300 tensors      G: ~1 M elements, many chunks
    # H: the lengths around one dword sweep and one 16-byte sweep of the kernel (and 4100: a whole sweep, one more group of four)
    seeded = [("chunk_edges", [CHUNK - 1, CHUNK, CHUNK + 1], [0, 0, 0], hyper_table(3, [(2e-3, 0.9, 5e-4)]), 11),
              ("three_hundred_tensors", [LENS[i % 10] if i < 100 else LENS[i % 7] for i in range(300)], [i % 2 for i in range(300)],
               hyper_table(3, [(2e-3, 0.9, 5e-4), (1e-3, 0.9, 1e-4)]), 12),
              ("long_tensor", [1000003], [0], hyper_table(3, [[(2e-3, 0.9, 5e-4), (2e-3, 0.9, 5e-4), (2e-4, 0.9, 5e-4)]]), 13),
              ("sweep_seams", [SWEEP1 - 1, SWEEP1, SWEEP1 + 1, SWEEP4 - 1, SWEEP4, SWEEP4 + 1, SWEEP4 + 4], [0] * 7, hyper_table(3, [(2e-3, 0.9, 5e-4)]), 14)]
    for name, lens, group, hyper, seed in seeded:
        p0, g = sgd_ref.seeded_inputs(seed, sum(lens), hyper.shape[0])
        cases.append((name, lens, group, hyper, p0, g, seed))
    kinds["lengths around the chunk"] = 2
    kinds["300 tensors"] = len(seeded[1][1])
    kinds["lengths around the sweeps"] = len(seeded[3][1])
    kinds["elements of the long tensor"] = seeded[2][1][0]

    out = {"n_cases": np.int64(len(cases))}
    n_sub = 0
    for i, c in enumerate(cases):
        name, lens, group, hyper, p0, g = c[:6]
        k = "c%d_" % i
        res = run_torch(lens, group, hyper, p0, g)
        out[k + "name"], out[k + "lens"], out[k + "group"], out[k + "hyper"] = np.str_(name), np.array(lens, np.int64), np.array(group, np.int32), hyper
        if len(c) == 7:
            assert sum(lens) >= KEEP_INPUTS_BELOW
            out[k + "seed"], out[k + "sha_p0"], out[k + "sha_g"] = np.int64(c[6]), np.str_(sgd_ref.sha(p0)), np.str_(sgd_ref.sha(g))
        else:
            assert sum(lens) < KEEP_INPUTS_BELOW
            out[k + "p0"], out[k + "g"] = p0, g
        out[k + "sha_p"] = np.array([sgd_ref.sha(r[0]) for r in res])
        out[k + "sha_m"] = np.array([sgd_ref.sha(r[1]) for r in res])
        out[k + "born"] = np.stack([r[2] for r in res])
        if sum(lens) < KEEP_FINAL_BELOW:
            out[k + "p_final"], out[k + "m_final"] = res[-1][0], res[-1][1]
        if name == "lengths_five_steps":                                   # products lr * m in the subnormal range, as the update forms them
            for s, r in enumerate(res):
                prod = np.abs(np.float64(np.float32(hyper[s, 0, 0])) * r[1].astype(np.float64))
                n_sub += int(((prod > 0) & (prod < 2.0 ** -126)).sum())
            assert all(r[2].all() for r in res) and np.isnan(res[-1][0]).sum() == 1
        if name == "momentum_zero":
            assert not any(r[2].any() for r in res)
        if name == "wd0_inf_parameter":
            assert np.isinf(res[-1][0]).sum() == 3 and not np.isnan(res[-1][0]).any()       # no 0 * inf anywhere
    kinds["subnormal lr * m products"] = n_sub
    for what, n in kinds.items():
        print("%-40s %d" % (what, n))
        assert n >= 1, what
    assert kinds["short lengths"] == 10 and kinds["300 tensors"] == 300 and kinds["zero gradients"] >= 4 and kinds["-0.0 gradients"] >= 4
    path = os.path.join(HERE, "sgd.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes, torch %s" % (path, os.path.getsize(path), torch.__version__))


if __name__ == "__main__":
    main()
