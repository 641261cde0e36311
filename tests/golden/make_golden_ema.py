"""Writes tests/golden/ema.npz from torch on the CPU (run by hand: python tests/golden/make_golden_ema.py).

  t<i>_*   torch._foreach_lerp_ trajectories of 12 updates: the average e starts at e0, update k lerps it towards p[k] with the float32
           weight w[k] of the schedule (tests/ema_ref.py: weight).  With warm-up and decay 0.9998 updates 0-8 take lerp's large-weight
           branch (w >= 0.5) and updates 9-11 the small one; without warm-up w = 2e-4 throughout; decay 0.3 without warm-up is w = 0.7
           throughout.  The tensors hold +-inf, NaN, -0 and subnormals beside ordinary values.
  mlp_*    a 2-layer MLP trained 12 steps with torch.optim.SGD (momentum 0.9, weight decay 5e-4) under MultiStepLR([4, 8]) with
           torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)); the averaged model takes one update_parameters()
           in front of the first step (its first call copies), so every later call is a lerp: initial weights, the gradient, the learning
           rate, the weights and the averaged weights of every step, flat in parameter order."""
import os

import numpy as np
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 12


def weight(decay, warmup, n):
    return np.float32(1.0 - (min(decay, (1 + n) / (10 + n)) if warmup else decay))


def special(rs, n):
    v = (rs.standard_normal(n) * 0.1).astype(np.float32)
    for i, s in zip(range(0, n, max(n // 9, 1)), (np.inf, -np.inf, np.nan, -0.0, 1e-40, -3e-39, 0.0, 1e-38, 3e38)):
        v[i] = np.float32(s)
    return v


def trajectory(out, i, name, decay, warmup, seed):
    rs = np.random.RandomState(seed)
    n = 1 + 3 + 4 + 5 + 257
    e0 = special(rs, n)
    p = np.stack([special(np.random.RandomState(seed + 100 + k), n) if k % 5 == 4 else (rs.standard_normal(n) * 0.1).astype(np.float32)
                  for k in range(STEPS)])
    p[3, ::7] = e0[::7]                                                     # d == 0, and inf - inf
    e = torch.from_numpy(e0.copy())
    es, ws = [], []
    for k in range(STEPS):
        w = weight(decay, warmup, k)
        torch._foreach_lerp_([e], [torch.from_numpy(p[k].copy())], float(w))
        es.append(e.numpy().copy()), ws.append(w)
    k = "t%d_" % i
    out.update({k + "name": np.array(name), k + "decay": np.float64(decay), k + "warmup": np.array(warmup), k + "p": p, k + "e0": e0,
                k + "e": np.stack(es), k + "w": np.array(ws, np.float32)})


def mlp(out, decay=0.9):
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(7, 16), torch.nn.ReLU(), torch.nn.Linear(16, 3))
    hyper = dict(lr=5e-2, momentum=0.9, weight_decay=5e-4)
    opt = torch.optim.SGD(model.parameters(), **hyper)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[4, 8], gamma=0.1)
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
    avg.update_parameters(model)                                            # the first call copies
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(STEPS, 8, 7, generator=g), torch.randn(STEPS, 8, 3, generator=g)
    flat = lambda ps, grad=False: np.concatenate([(q.grad if grad else q).detach().numpy().reshape(-1) for q in ps]).astype(np.float32)  # noqa: E731
    p0 = flat(model.parameters())
    gs, ps, es, lrs = [], [], [], []
    for k in range(STEPS):
        opt.zero_grad()
        torch.nn.functional.mse_loss(model(x[k]), y[k]).backward()
        gs.append(flat(model.parameters(), True)), lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        avg.update_parameters(model)
        sched.step()
        ps.append(flat(model.parameters())), es.append(flat(avg.module.parameters()))
    out.update(mlp_decay=np.float64(decay), mlp_shapes=np.array([list(q.shape) + [0] * (2 - q.dim()) for q in model.parameters()], np.int64),
               mlp_hyper=np.array([hyper["lr"], hyper["momentum"], hyper["weight_decay"]], np.float64), mlp_lr=np.array(lrs, np.float64),
               mlp_p0=p0, mlp_g=np.stack(gs), mlp_p=np.stack(ps), mlp_e=np.stack(es))


def main():
    out = {}
    trajectory(out, 0, "warmup_0p9998", 0.9998, True, 11)
    trajectory(out, 1, "plain_0p9998", 0.9998, False, 12)
    trajectory(out, 2, "plain_0p3", 0.3, False, 13)
    out["n_traj"] = np.int64(3)
    mlp(out)
    path = os.path.join(HERE, "ema.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
