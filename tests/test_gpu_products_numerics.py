"""Both product forms of the fp32 conv stage (csrc/rpn_conv_f32.hip, rpn_wino_gemm_kernel; ops.conv3x3_f32_products) on ADVERSE operands against float64.

The other tests of the stage draw zero-mean randn operands, where the rounding of a long sum cancels.  Here the operands are the ones where a product
form that is subtly wrong shows: all-positive sums at conv5 depth (K = 4 608) and at FPN P2's 1 x 1 weight-gradient length (K = 67 200), magnitudes
spread over 2^+-40, cancellation-heavy sums, post-ReLU activations, long all-positive weight-gradient sums, and channel scales of 2^+-20.  The GEMM
cases go through ops.gemm_nt (frcnn_gemm_nt_f32: the same kernel, the 1 x 1 weight gradients), the convolutions through conv3x3_fwd / _bwd_data /
_wgrad.

Error metric, per output, in float64 on the CPU: r = the exact result, S = sum |terms| (|A| . |B|^T for the GEMM; for a convolution the same
convolution of |x| and |w| (|dy|), plus |b|), eps = (out - r) / S; where S == 0 the output must be exactly 0.  Per case and form: max |eps|,
rms(eps), mean(eps) (printed per case, one JSON line each -- run with -s to see them; the table in docs/PARITY.md (e')).  Asserted:
  (a) max |eps| <= C_op * u * sqrt(K), u = 2^-24, K = the contraction length of the DIRECT operation (GEMM: K; forward: 9 Cin; data gradient: 9 Cout;
      weight gradient: H W).  C_op is the largest max |eps| / (u sqrt(K)) the NATIVE form showed over this module's cases on its first measured run,
      times at least 2 (the measured values are beside each constant below).  sqrt(K): a long fp32 sum's rounding error grows as its square root
      when the roundings are unbiased -- which is exactly what a biased form violates at large K.
  (b) split's max and rms eps are each <= 1.5 x native's + u, on the same data.
  (c) DC: |mean eps| of split <= |mean eps| of native + 4 std(eps) / sqrt(n_eff) (std: the larger of the two forms'), the statistic of
      tools/dev/micro/split_dc_check.hip.  Outputs that share an operand row share that row's rounding history, so they are not independent draws: n_eff
      counts only outputs with pairwise disjoint operands -- min(M, N) for the GEMM (a diagonal), min(Cout, Cin) for the weight gradient, and
      min(channels, H W / 9) for forward and data gradient (3 x 3 windows that do not overlap).

The kernels are bit-reproducible, so every seeded case is deterministic; the margins are still honest ones, not fits to the last digit.

Not tested as split: 64 -> 64 layers on 4 x 4 tiles run rpn_wino_gemm_out64_kernel (products and output transform fused), which has no split
instantiation -- its products are v_mfma_f32_16x16x4_f32 whatever the switch says (rpn_conv_f32.hip, frcnn_conv3x3_f32_fwd / _bwd_data dispatch).

Bit-exact cut: with B one-hot (O[i, j] = A[i, pi(j)]), both forms must return A's values bit for bit, for fp32 bit patterns over every finite exponent,
+-0, the largest finite value, the smallest normal, subnormals, all-ones mantissas and low halves 0x8000 / 0x7FFF / 0xFFFF: a wrong m or l piece of
the split cut (wn_cut8) shows there, in the shipped kernel's own register context.  SPLIT_EXACT_MIN is the smallest |v| at which the split form is
exact (see that constant).

The split form's all-positive cases failed (c) when this module was written: mean eps -3.5e-8 (-0.6 u) against native's +-7e-10, at every K and tile
shape.  The cause was the cut (wn_cut8): with the pieces truncated, all three carried v's sign and so did the three products the form drops (m l, l m,
l l, about 2^-25 of the term together).  m is now rounded to nearest, which leaves l of either sign."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24

# (a)'s constants: C_op, in units of u * sqrt(K).  The native form's first measured run gave as its largest max|eps| / (u sqrt K): gemm 0.056 (spread,
# 192 x 192), forward 2.06 (channel_spread), data gradient 1.69 (channel_spread), weight gradient 0.41 (conv5); each constant is about 2.1 x that.  The
# convolutions' constants are larger than the GEMM's: F(4 x 4, 3 x 3)'s transforms (constants 1/24 .. 8) multiply the products' rounding before it reaches y.
C_BOUND = {"gemm": 0.12, "fwd": 4.5, "bwd_data": 3.5, "wgrad": 0.85}
# The split cut is exact for |v| >= 2^-110 (and 0).  Below, its third piece l (~2^-16 |v|) falls under fp32's normal range and the cut loses it: measured
# on the first run, every miss was below 2^-110 in magnitude and off by far less than the smallest normal (the bound asserted there).  The native
# form is exact everywhere, subnormals included.
SPLIT_EXACT_MIN = 2.0 ** -110


@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


@pytest.fixture
def products(request, ops):
    """The product form under test (parametrised through FORMS: native and split, case by case so that both share the float64 reference), set for
    the test and restored after it."""
    assert ops.conv3x3_f32_products() == "native"
    prev = ops.conv3x3_f32_products(request.param)
    try:
        yield request.param
    finally:
        ops.conv3x3_f32_products(prev)


FORMS = pytest.mark.parametrize("products", ["native", "split"], indirect=True)


def _native(ops, fn):
    """fn() under the native form, whatever the current one; the current one is put back."""
    prev = ops.conv3x3_f32_products("native")
    try:
        return fn()
    finally:
        ops.conv3x3_f32_products(prev)


def _stats(out, r, S):
    out = out.detach().double().cpu()
    zero = S == 0
    assert torch.equal(out[zero], torch.zeros_like(out[zero])), "outputs whose terms are all 0 must be exactly 0"
    eps = ((out - r) / torch.where(zero, torch.ones_like(S), S))[~zero]
    return {"max": float(eps.abs().max()), "rms": float(eps.pow(2).mean().sqrt()), "mean": float(eps.mean()), "std": float(eps.std())}


def _record(name, rec):
    print("\n[products %s] %s" % (name, json.dumps(rec, sort_keys=True)))


def _measure(name, op, K, n_eff, mode, st, nat):
    rec = {"name": name, "mode": mode, "op": op, "K": K, "n_eff": n_eff, "native": nat, mode: st, "bound_a": C_BOUND[op] * U * math.sqrt(K)}
    _record("%s-%s" % (name, mode), rec)
    return rec


def _check(rec):
    """(a) for this form; (b) and (c) against the native form's stats on the same data when this form is split."""
    name, mode, n_eff, st, nat = rec["name"], rec["mode"], rec["n_eff"], rec[rec["mode"]], rec["native"]
    assert st["max"] <= rec["bound_a"], ("(a)", name, mode, rec)
    if mode == "split":
        assert st["max"] <= 1.5 * nat["max"] + U and st["rms"] <= 1.5 * nat["rms"] + U, ("(b)", name, rec)
        noise = 4.0 * max(st["std"], nat["std"]) / math.sqrt(n_eff)
        assert abs(st["mean"]) <= abs(nat["mean"]) + noise, ("(c)", name, rec, noise)


_REF = {}


def _ref(key, make):
    """The float64 references of the last case (native and split of one case run next to each other: computed once)."""
    if key not in _REF:
        _REF.clear()
        _REF[key] = make()
    return _REF[key]


# ---- GEMM: ops.gemm_nt, O = A . B^T ----
def _gemm_operands(kind, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "mixed":
        return torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    if kind == "all_positive":
        return torch.rand(M, K, generator=g), torch.rand(N, K, generator=g)
    if kind == "spread":                                   # random sign x [1, 2) x 2^e, e uniform in [-40, 40] per element (full mantissas: all three pieces)
        def f(R):
            e = torch.randint(-40, 41, (R, K), generator=g).double()
            s = torch.randint(0, 2, (R, K), generator=g).double() * 2 - 1
            return (s * (1 + torch.rand(R, K, generator=g).double()) * torch.exp2(e)).float()
        return f(M), f(N)
    if kind == "spread_rows":                              # per-row (A) and per-column (B) scales of 2^+-40
        ra = torch.exp2(torch.randint(-40, 41, (M, 1), generator=g).double()).float()
        rb = torch.exp2(torch.randint(-40, 41, (N, 1), generator=g).double()).float()
        return torch.randn(M, K, generator=g) * ra, torch.randn(N, K, generator=g) * rb
    if kind == "cancel_zero":                              # A = [a, a], B = [b, -b]: exactly 0
        a, b = torch.randn(M, K // 2, generator=g), torch.randn(N, K // 2, generator=g)
        return torch.cat([a, a], 1), torch.cat([b, -b], 1)
    if kind == "cancel_rem":                               # large +- pairs (2^10) and a small remainder (2^-10) that the exact result is made of
        k2, kr = (K - 512) // 2, 512
        a, b = torch.randn(M, k2, generator=g) * 1024, torch.randn(N, k2, generator=g) * 1024
        c, d = torch.randn(M, kr, generator=g) / 1024, torch.randn(N, kr, generator=g) / 1024
        return torch.cat([a, a, c], 1), torch.cat([b, -b, d], 1)
    raise ValueError(kind)


GEMM_CASES = [(kind, K) for kind, Ks in (("mixed", (4608, 67200)), ("all_positive", (4608, 67200)), ("spread", (4608,)), ("spread_rows", (4608,)),
                                         ("cancel_zero", (4608,)), ("cancel_rem", (4608,))) for K in Ks]
MN = [(128, 128), (128, 192), (192, 128), (192, 192)]          # all four NT tile instantiations: 128 / 64 x 128 / 64


@FORMS
@pytest.mark.parametrize("kind,K", GEMM_CASES, ids=["%s_K%d" % c for c in GEMM_CASES])
def test_gemm_nt_products_vs_float64_on_adverse_operands(ops, products, kind, K):
    """ops.gemm_nt on every (M, N) in {128, 192}^2 (each a split-K product: _gemm_nt_splits > 1 at these K), eps against float64: (a), (b), (c)."""
    recs = []
    for M, N in MN:
        assert ops._gemm_nt_splits(M, N, K) > 1
        name = "gemm_%s_K%d_%dx%d" % (kind, K, M, N)
        a, b = _gemm_operands(kind, M, N, K, seed=K + 7 * M + N + len(kind))
        r, S = _ref(name, lambda: (a.double() @ b.double().T, a.double().abs() @ b.double().abs().T))
        ad, bd = a.to(DEV), b.to(DEV)
        out = ops.gemm_nt(ad, bd)
        assert torch.equal(out, ops.gemm_nt(ad, bd))                                       # bit-reproducible
        st = _stats(out, r, S)
        nat = st if products == "native" else _stats(_native(ops, lambda: ops.gemm_nt(ad, bd)), r, S)
        recs.append(_measure(name, "gemm", K, min(M, N), products, st, nat))
    for rec in recs:                                                                           # every shape measured (and recorded) first
        _check(rec)


# ---- the cut: one-hot operands return the other operand's values bit for bit ----
def _patterns(n, seed):
    """n fp32 values (as float32 tensor): raw bit patterns over every finite exponent and the edge values."""
    rng = np.random.RandomState(seed)
    bits = rng.randint(0, 1 << 31, size=n, dtype=np.int64).astype(np.uint32)
    bits = (bits & np.uint32(0x807FFFFF)) | (np.uint32(rng.randint(0, 255, size=n)) << np.uint32(23))      # exponent field 0 .. 254
    bits ^= np.uint32(rng.randint(0, 2, size=n)) << np.uint32(31)
    edge = [0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00400000, 0x00008000,
            0x3F800000, 0x3FFFFFFF, 0xBF7FFFFF]
    edge += [(e << 23) | 0x7FFFFF for e in range(0, 255, 3)]                                   # all-ones mantissas
    edge += [(e << 23) | hi | lo for e in range(1, 255, 5) for hi in (0x000000, 0x7F0000, 0x550000) for lo in (0x8000, 0x7FFF, 0xFFFF)]   # low halves
    edge = np.array(edge, dtype=np.uint32)
    bits[: len(edge)] = edge
    bits[len(edge): 2 * len(edge)] = edge ^ np.uint32(0x80000000)
    return torch.from_numpy(bits.view(np.float32).copy())


@FORMS
@pytest.mark.parametrize("K", [32, 4608, 67200])
def test_gemm_nt_one_hot_returns_the_operand_bit_for_bit(ops, products, K):
    """B one-hot: O[i, j] = A[i, pi(j)] exactly (and the same with the roles swapped, for the B side's cut), under both forms; K = 32 is one piece,
    4 608 and 67 200 are split-K products.  Under split, values below SPLIT_EXACT_MIN in magnitude are held to (a)'s form of bound instead."""
    M, N = 192, 128
    g = torch.Generator().manual_seed(K)
    vals = _patterns(M * K, seed=K)
    a = vals.view(M, K)
    pi = torch.randperm(K, generator=g)[:N] if N <= K else torch.randint(0, K, (N,), generator=g)
    oh = torch.zeros(N, K)
    oh[torch.arange(N), pi] = 1.0
    want = a[:, pi]
    got = ops.gemm_nt(a.to(DEV), oh.to(DEV)).cpu()
    got_t = ops.gemm_nt(oh.to(DEV), a.to(DEV)).cpu()                                             # the one-hot operand on the A side
    bad = [(float(w), float(x)) for w, x in zip(want.flatten().tolist(), got.flatten().tolist()) if not (w == x)]
    bad_t = [(float(w), float(x)) for w, x in zip(want.T.flatten().tolist(), got_t.flatten().tolist()) if not (w == x)]
    _record("cut_K%d-%s" % (K, products), {"n": want.numel(), "bad": len(bad), "bad_t": len(bad_t), "bad_abs_max": max([abs(w) for w, _ in bad + bad_t], default=0.0),
                                            "first": (bad + bad_t)[:20],
                                            "err_max": max([abs(w - x) for w, x in bad + bad_t], default=0.0)})
    exact = want.abs() >= (SPLIT_EXACT_MIN if products == "split" else 0.0)
    assert torch.equal(got[exact], want[exact]) and torch.equal(got_t[exact.T], want.T[exact.T])
    if not bool(exact.all()):                                                                  # below the domain: off by less than the smallest normal
        assert float((got[~exact] - want[~exact]).abs().max()) < 2.0 ** -126
        assert float((got_t[~exact.T] - want.T[~exact.T]).abs().max()) < 2.0 ** -126


# ---- convolutions: conv3x3_fwd (bias, no ReLU), conv3x3_bwd_data (no mask), conv3x3_wgrad ----
def _conv_operands(kind, Cin, Cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind in ("relu_zero_mean_w", "relu_positive_w"):
        x = torch.relu(torch.randn(1, Cin, H, W, generator=g) + 0.5)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
        if kind == "relu_zero_mean_w":
            w = w - w.mean(dim=(1, 2, 3), keepdim=True)                                     # every filter sums to ~0: heavy cancellation
        else:
            w = w.abs() * 0.5 + w * 0.5                                                     # positive-mean filters
        dy = torch.randn(1, Cout, H, W, generator=g)
    elif kind == "long_k":
        x = torch.relu(torch.randn(1, Cin, H, W, generator=g) + 0.5)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
        dy = torch.rand(1, Cout, H, W, generator=g)
    elif kind == "channel_spread":
        ex = torch.randint(-20, 21, (1, Cin, 1, 1), generator=g).double()
        ew = torch.randint(-20, 21, (Cout, 1, 1, 1), generator=g).double()
        x = torch.randn(1, Cin, H, W, generator=g) * torch.exp2(ex).float()
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * torch.exp2(ew).float() * (2.0 / (9 * Cin)) ** 0.5
        dy = torch.randn(1, Cout, H, W, generator=g)
    else:
        raise ValueError(kind)
    b = torch.randn(Cout, generator=g) * 0.2
    return x, w, b, dy


CONV_CASES = [   # id, operand kind, Cin, Cout, H, W, ops
    ("conv5_zero_mean_w", "relu_zero_mean_w", 512, 512, 37, 62, ("fwd", "bwd_data", "wgrad")),
    ("conv5_positive_w", "relu_positive_w", 512, 512, 37, 62, ("fwd", "bwd_data")),
    ("conv4_2_zero_mean_w", "relu_zero_mean_w", 512, 512, 75, 125, ("fwd", "bwd_data", "wgrad")),
    ("conv4_2_positive_w", "relu_positive_w", 512, 512, 75, 125, ("fwd", "bwd_data")),
    ("c128_256_zero_mean_w", "relu_zero_mean_w", 128, 256, 150, 250, ("fwd", "bwd_data", "wgrad")),
    ("c128_256_positive_w", "relu_positive_w", 128, 256, 150, 250, ("fwd", "bwd_data")),
    ("wgrad_64_128_300x500", "long_k", 64, 128, 300, 500, ("wgrad",)),
    ("wgrad_128_128_300x500", "long_k", 128, 128, 300, 500, ("wgrad",)),
    ("channel_spread", "channel_spread", 256, 256, 50, 84, ("fwd", "bwd_data", "wgrad")),
]
CONV_OPS = [(c[0],) + c[1:6] + (op,) for c in CONV_CASES for op in c[6]]


def _conv_ref(op, x, w, b, dy):
    x, w, b, dy = x.double(), w.double(), b.double(), dy.double()
    if op == "fwd":
        return F.conv2d(x, w, b, padding=1), F.conv2d(x.abs(), w.abs(), b.abs(), padding=1)
    if op == "bwd_data":
        return F.conv_transpose2d(dy, w, None, padding=1), F.conv_transpose2d(dy.abs(), w.abs(), None, padding=1)
    return (torch.nn.grad.conv2d_weight(x, tuple(w.shape), dy, padding=1),
            torch.nn.grad.conv2d_weight(x.abs(), tuple(w.shape), dy.abs(), padding=1))


@FORMS
@pytest.mark.parametrize("name,kind,Cin,Cout,H,W,op", CONV_OPS, ids=["%s-%s" % (c[0], c[-1]) for c in CONV_OPS])
def test_conv3x3_products_vs_float64_on_adverse_operands(ops, products, name, kind, Cin, Cout, H, W, op):
    """One operation of the stage on post-ReLU / long-K / channel-spread operands, eps against float64 with S from |x|, |w| (|dy|), |b|: (a), (b), (c)."""
    x, w, b, dy = _conv_operands(kind, Cin, Cout, H, W, seed=Cin + 3 * Cout + H + len(kind))
    r, S = _ref((name, op), lambda: _conv_ref(op, x, w, b, dy))
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    run = {"fwd": lambda: ops.conv3x3_fwd([xd], wd, bd)[0],
           "bwd_data": lambda: ops.conv3x3_bwd_data([dyd], wd)[0],
           "wgrad": lambda: ops.conv3x3_wgrad([xd], [dyd])[0]}[op]
    out = run()
    assert torch.equal(out, run())                                                             # bit-reproducible
    st = _stats(out, r, S)
    nat = st if products == "native" else _stats(_native(ops, run), r, S)
    K = {"fwd": 9 * Cin, "bwd_data": 9 * Cout, "wgrad": H * W}[op]
    n_eff = min(Cout, Cin) if op == "wgrad" else min(Cout if op == "fwd" else Cin, H * W // 9)
    _check(_measure("conv_%s_%s" % (name, op), op, K, n_eff, products, st, nat))
