"""The bf16 kernels of the mixed-precision configuration (BASELINE configs[4]) BIT FOR BIT, on data where arithmetic is exact.

Operands are small integers times one power of two ("dyadic").  Every product of two such bf16 values is exact in fp32, and every
partial sum -- in ANY order -- is exact as long as the sum of the absolute terms stays below 2^24 units; the fp32 accumulator of a
kernel then equals the float64 result, and the kernel's output must equal the float64 reference, rounded where the kernel says it
rounds, in every bit.  There is no tolerance in this file.  The rounding points, as the kernel headers state them:

  csrc/rpn_conv.hip (ops.rpn_conv_head_levels, rpn_conv_bwd_data, rpn_conv_wgrad, conv3x3_bf16_c256)
    packing      : W3, Wc, Wr fp32 -> bf16, round to nearest even (weights 257, 259, .. are planted so that this rounding, ties
                   included, is exercised)
    raw          = bf16(acc)                         stored for the backward
    h            = bf16(relu(float(raw) + b3))       the bias meets the ROUNDED raw; a NaN stays a NaN
    cls / reg    = fp32 sums of bf16(W) * h + fp32 bias
    bwd-data     = bf16(sum bf16(W3) * d_raw); conv3x3_bf16_c256 = that kernel on the flipped, transposed weight, its bf16 bias
                   added to the ROUNDED output in bf16 (one more rounding)
    wgrad        = fp32 sum of x * d_raw
  csrc/rpn_head.hip (ops.rpn_head_tail_levels(mfma="bf16") and the backward both heads share)
    forward      : as h / cls / reg above
    backward     : z = float(raw) + b3; dz = (z > 0) * sum_j W[j, c] g[p, j] with the fp32 (UNROUNDED) head weights on the fp32
                   matrix instruction; d_raw = bf16(dz); db3 = sum of the fp32 dz; dW = sum g * relu(z) with the fp32 (unrounded) h

Every test asserts its own preconditions on the float64 side (sums of absolute terms < 2^24 units, rounded intermediates normal,
counts of rounded values / ties / exact zeros > 0), repeats its call and asserts the second result identical.  The tests without
the gpu marker run the same reference on the CPU and prove the premise (an fp32 evaluation in another order gives the same bits)."""
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
C_, A = 256, 3
LIMIT = float(2 ** 24)
gpu = pytest.mark.gpu

FPN = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]           # the five levels of an 800 x 1344 frame: 89 523 positions
SHAPE_SETS = {                                                         # tile = 256 channels x 8 rows x 32 columns, levels share one launch
    "fpn800x1344": FPN,
    "widths": [(9, 31), (9, 32), (9, 33), (9, 64), (9, 65)],
    "heights": [(7, 40), (8, 40), (9, 40), (16, 40), (17, 40)],
    "tiny": [(1, 1), (1, 40), (40, 1)],
    "one_level": [(17, 33)],
    "smallest_first": [(3, 4), (40, 56), (5, 7), (20, 28), (10, 14)],  # offsets not monotone in size
    "twins": [(12, 33), (12, 33)],
}
SMALL_SETS = [k for k in SHAPE_SETS if k != "fpn800x1344"]
# exponents (activations, 3x3 weight, head weights, upstream gradient): integers, and one realistic magnitude.  A power-of-two rescale
# must not change a single mantissa bit.
SCALES = {"s0": (0, 0, 0, 0), "real": (3, 7, 6, 5)}


# ------------------------------------------------------------------------------------------ data
def dyadic(gen, shape, lo, hi, s=0, keep=1.0):
    """Seeded integers in [lo, hi] times 2^-s (float64, CPU); keep < 1 zeroes the others."""
    t = torch.randint(lo, hi + 1, shape, generator=gen).double()
    if keep < 1.0:
        t = t * (torch.rand(shape, generator=gen) < keep)
    return t * 2.0 ** -s


def plant_wide(gen, w, rows, per_row):
    """Odd integers 257 .. 265 (+-) at `per_row` places of each listed row of w [rows, ...] (units of the tensor's own scale are applied
    by the caller): not representable in bf16 and exactly half way between two neighbours -- the packing kernels' rounding decides."""
    flat = w.reshape(w.shape[0], -1)
    for r in rows:
        idx = torch.randperm(flat.shape[1], generator=gen)[:per_row]
        val = 257 + 2 * torch.randint(0, 5, (per_row,), generator=gen)
        sign = 1 - 2 * torch.randint(0, 2, (per_row,), generator=gen)
        flat[r, idx] = (val * sign).double()
    return w


def bf(t):
    """Round a float64 tensor of fp32-representable values to bf16 (nearest even), back in float64."""
    return t.float().bfloat16().double()


def make_head_case(shapes, scale, seed=0):
    """Feature maps, the head's parameters and upstream gradients (all float64 on the CPU) in the issue's ranges: activations [-4, 4],
    weights [-2, 2] (+ a few planted 257 .. 265), biases [-4, 4], gradients [-2, 2], sparse when there are many positions."""
    sx, sw, sh, sg = SCALES[scale]
    gen = torch.Generator().manual_seed(1000 + seed)
    P = sum(h * w for h, w in shapes)
    d = {"shapes": list(shapes), "u_raw": 2.0 ** -(sx + sw), "u_out": 2.0 ** -(sx + sw + sh), "u_g": 2.0 ** -sg, "u_dz": 2.0 ** -(sg + sh),
         "u_x": 2.0 ** -sx, "u_w3": 2.0 ** -sw, "u_wh": 2.0 ** -sh}
    d["feats"] = [dyadic(gen, (1, C_, h, w), -4, 4, sx) for h, w in shapes]
    w3 = plant_wide(gen, dyadic(gen, (C_, C_, 3, 3), -2, 2), range(3, C_, 8), 4)           # 32 of the 256 output channels carry wide weights
    d["w3"] = w3 * 2.0 ** -sw
    d["b3"] = dyadic(gen, (C_,), -4, 4, sx + sw)
    d["wc"] = plant_wide(gen, dyadic(gen, (2 * A, C_), -2, 2), range(2 * A), 1) * 2.0 ** -sh
    d["wr"] = plant_wide(gen, dyadic(gen, (4 * A, C_), -2, 2), range(4 * A), 1) * 2.0 ** -sh
    d["bc"] = dyadic(gen, (2 * A,), -4, 4, sx + sw + sh)
    d["br"] = dyadic(gen, (4 * A,), -4, 4, sx + sw + sh)
    keep = 1.0 if P < 20000 else 0.125                       # the head weight gradient sums g * h over all positions: keep it below 2^24 units
    d["gc"] = dyadic(gen, (1, P * A, 2), -2, 2, sg, keep)
    d["gr"] = dyadic(gen, (1, P * A, 4), -2, 2, sg, keep)
    return d


# ------------------------------------------------------------------------------------------ preconditions
def need_exact(abs_sum, unit, what):
    """The sum of the absolute terms of every output, in units of the output's grid, must stay below 2^24: then any fp32 summation order is exact."""
    m = float(abs_sum.max()) / unit
    assert m < LIMIT, "%s: largest sum of absolute terms %.0f units >= 2^24 -- narrow the ranges" % (what, m)
    return m


def need_normal(t, what):
    """Every value fed on is finite and zero or a normal fp32 / bf16 number (both have 8 exponent bits)."""
    a = t.abs()
    assert bool(torch.isfinite(t).all()) and (not bool((a > 0).any()) or float(a[a > 0].min()) >= 2.0 ** -126), what


def bf16_ties(v):
    """How many values lie exactly half way between two bf16 neighbours: with |v| = m 2^e, m in [0.5, 1), the bf16 grid has spacing 2^-8 in m
    (exact arithmetic on the float64 mantissa, no power function involved)."""
    m, _ = torch.frexp(v.abs())
    x = m * 256.0
    return int(((x - x.floor()) == 0.5).sum())


# ------------------------------------------------------------------------------------------ float64 references
def conv64(x, w, dtype=torch.float64):
    return F.conv2d(x.to(dtype), w.to(dtype), None, padding=1).double()


def tail_forward_ref(raws, d, stats):
    """h = bf16(relu(raw + b3)); cls / reg = bf16(W) h + bias, in the NHWC / concatenated layout.  raws: float64 [1,C,h,w] of bf16 values."""
    wc, wr = bf(d["wc"]), bf(d["wr"])
    cls, reg, zs = [], [], []
    for raw in raws:
        z = raw + d["b3"].view(1, -1, 1, 1)
        hr = torch.relu(z)
        h = bf(hr)
        need_normal(h, "h")
        stats["z_zero"] += int((z == 0).sum()); stats["h_rounded"] += int((h != hr).sum()); stats["h_ties"] += bf16_ties(hr)
        both = torch.cat([wc, wr], 0)[:, :, None, None]
        out = F.conv2d(h, both, torch.cat([d["bc"], d["br"]]))
        stats["out_abs"] = max(stats["out_abs"], need_exact(F.conv2d(h, both.abs(), torch.cat([d["bc"], d["br"]]).abs()), d["u_out"], "cls / reg"))
        need_exact(raw.abs() + d["b3"].abs().view(1, -1, 1, 1), d["u_raw"], "raw + b3")
        out = out.permute(0, 2, 3, 1)
        cls.append(out[..., :2 * A].reshape(1, -1, 2)); reg.append(out[..., 2 * A:].reshape(1, -1, 4)); zs.append(z)
    return torch.cat(cls, 1), torch.cat(reg, 1), zs


def tail_backward_ref(zs, d, stats):
    """d_raw (bf16), dWc / dWr, dbc / dbr, db3 of the shared tail backward from z = raw + b3 per level."""
    w_all = torch.cat([d["wc"], d["wr"]], 0)                  # fp32 weights, NOT rounded: the backward's fp32 matrix instruction reads them as they are
    dW = torch.zeros(6 * A, C_, dtype=torch.float64, device=w_all.device)
    dW_abs, db, db3, db3_abs = torch.zeros_like(dW), torch.zeros(6 * A, dtype=torch.float64, device=w_all.device), 0, 0
    d_raws, p0 = [], 0
    for z in zs:
        _, _, hh, ww = z.shape
        P = hh * ww
        gg = torch.cat([d["gc"].reshape(-1, 2 * A)[p0:p0 + P], d["gr"].reshape(-1, 4 * A)[p0:p0 + P]], 1)      # [P, 18]
        zz = z.reshape(C_, P)
        mask = (zz > 0).double()
        full = w_all.t() @ gg.t()
        dz = full * mask
        need_exact(w_all.abs().t() @ gg.abs().t(), d["u_dz"], "dz")
        hr = torch.relu(zz)
        dW += gg.t() @ hr.t(); dW_abs += gg.abs().t() @ hr.t()
        db += gg.sum(0); db3 = db3 + dz.sum(1); db3_abs = db3_abs + dz.abs().sum(1)
        dr = bf(dz)
        need_normal(dr, "d_raw")
        stats["dz_masked_at_zero"] += int(((zz == 0) & (full != 0)).sum())
        d_raws.append(dr.reshape(1, C_, hh, ww))
        p0 += P
    stats["dW_head_abs"] = need_exact(dW_abs, d["u_g"] * d["u_raw"], "head weight gradient")
    need_exact(db3_abs, d["u_dz"], "db3")
    return d_raws, dW[:2 * A], db[:2 * A], dW[2 * A:], db[2 * A:], db3


def wgrad_ref(feats, d_raws, unit, stats):
    """dW3 = sum over levels and positions of d_raw * x (float64 autograd of the convolution), with its sum of absolute terms."""
    out = []
    for fs, ds in ((feats, d_raws), ([f.abs() for f in feats], [t.abs() for t in d_raws])):
        w = torch.zeros(C_, C_, 3, 3, dtype=torch.float64, device=feats[0].device, requires_grad=True)
        sum((F.conv2d(f, w, None, padding=1) * t).sum() for f, t in zip(fs, ds)).backward()
        out.append(w.grad)
    stats["dW3_abs"] = need_exact(out[1], unit, "3x3 weight gradient")
    return out[0]


def bwd_data_ref(d_raws, w3, unit, stats=None):
    """bf16(conv_transpose(d_raw, bf16(W3))) per level."""
    w3r = bf(w3)
    outs = []
    for t in d_raws:
        need_exact(F.conv_transpose2d(t.abs(), w3r.abs(), padding=1), unit, "data gradient")
        acc = F.conv_transpose2d(t, w3r, padding=1)
        o = bf(acc)
        need_normal(o, "d_x")
        if stats is not None:
            stats["dx_rounded"] = stats.get("dx_rounded", 0) + int((o != acc).sum()); stats["dx_ties"] = stats.get("dx_ties", 0) + bf16_ties(acc)
        outs.append(o)
    return outs


def new_stats():
    return {"z_zero": 0, "h_rounded": 0, "h_ties": 0, "raw_big": 0, "raw_rounded": 0, "raw_ties": 0, "out_abs": 0.0, "raw_abs": 0.0, "dz_masked_at_zero": 0}


def head_reference(d, dev, conv_dtype=torch.float64, backward=True):
    """Everything ops.rpn_conv_head_levels computes, forward and backward, in float64 on `dev` with the kernel's rounding points."""
    d = {k: ([t.to(dev) for t in v] if k == "feats" else (v.to(dev) if torch.is_tensor(v) else v)) for k, v in d.items()}
    st = new_stats()
    w3r = bf(d["w3"])
    st["w3_rounded"] = int((w3r != d["w3"]).sum()); st["w3_ties"] = bf16_ties(d["w3"])
    raws = []
    for f in d["feats"]:
        acc = conv64(f, w3r, conv_dtype)
        st["raw_abs"] = max(st["raw_abs"], need_exact(conv64(f.abs(), w3r.abs(), conv_dtype), d["u_raw"], "raw"))
        raw = bf(acc)
        need_normal(raw, "raw")
        st["raw_big"] += int((acc.abs() > 256 * d["u_raw"]).sum()); st["raw_rounded"] += int((raw != acc).sum()); st["raw_ties"] += bf16_ties(acc)
        raws.append(raw)
    cls, reg, zs = tail_forward_ref(raws, d, st)
    ref = {"raws": raws, "cls": cls, "reg": reg, "stats": st}
    if backward:
        d_raws, dwc, dbc, dwr, dbr, db3 = tail_backward_ref(zs, d, st)
        ref.update(d_raws=d_raws, dwc=dwc, dbc=dbc, dwr=dwr, dbr=dbr, db3=db3)
        ref["d_feats"] = bwd_data_ref(d_raws, d["w3"], d["u_dz"] * d["u_w3"])
        ref["dw3"] = wgrad_ref(d["feats"], d_raws, d["u_dz"] * d["u_x"], st)
    return ref


def assert_not_vacuous(st):
    """(b) the bf16 roundings, ties included, are exercised and (c) pre-activations equal to exactly zero occur."""
    assert st["raw_big"] > 0 and st["raw_rounded"] > 0 and st["raw_ties"] > 0, st
    assert st["h_rounded"] > 0 and st["h_ties"] > 0 and st["z_zero"] > 0, st
    assert st["w3_rounded"] > 0 and st["w3_ties"] > 0, st


def same_bits(got, ref, what):
    """got (device tensor, fp32 or bf16) equals the float64 reference exactly: the reference must be representable in got's type, and then
    equal values are equal bit patterns (the sign of a zero aside, which no sum of exact terms defines)."""
    want = ref.to(got.device).to(got.dtype)
    assert torch.equal(want.double(), ref.to(got.device)), what + ": the reference is not representable in the output type"
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (what, bad.shape[0], got.numel(), i, float(got[i]), float(want[i])))


# ------------------------------------------------------------------------------------------ CPU self-checks (no GPU)
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("name", SMALL_SETS)
def test_cpu_premise_float32_in_another_order_equals_float64(name, scale):
    """On the generator's data an fp32 CPU convolution (its own blocking and summation order) equals the float64 one in every bit, the
    preconditions hold and the interesting cases (rounded values, ties, exact zeros) occur -- before any kernel is involved."""
    d = make_head_case(SHAPE_SETS[name], scale)
    ref = head_reference(d, "cpu")
    assert_not_vacuous(ref["stats"])
    ref32 = head_reference(d, "cpu", conv_dtype=torch.float32, backward=False)
    for a, b in zip(ref["raws"], ref32["raws"]):
        assert torch.equal(a, b)
    assert torch.equal(ref["cls"], ref32["cls"]) and torch.equal(ref["reg"], ref32["reg"])
    w3r = bf(d["w3"])
    for f, g_, dx in zip(d["feats"], ref["d_raws"], ref["d_feats"]):
        assert torch.equal(F.conv2d(f.float(), w3r.float(), None, padding=1).double(), F.conv2d(f, w3r, None, padding=1))
        assert torch.equal(bf(F.conv_transpose2d(g_.float(), w3r.float(), padding=1).double()), dx)
    f, t = d["feats"][0], ref["d_raws"][0]
    dw32 = torch.nn.grad.conv2d_weight(f.float(), (C_, C_, 3, 3), t.float(), padding=1).double()
    assert torch.equal(dw32, torch.nn.grad.conv2d_weight(f, (C_, C_, 3, 3), t, padding=1))


def test_cpu_power_of_two_rescale_changes_no_mantissa_bit():
    a, b = head_reference(make_head_case(SHAPE_SETS["one_level"], "s0"), "cpu"), head_reference(make_head_case(SHAPE_SETS["one_level"], "real"), "cpu")
    sx, sw, sh, sg = SCALES["real"]
    for k, s in (("cls", sx + sw + sh), ("reg", sx + sw + sh), ("dw3", sg + sh + sx), ("dwc", sg + sx + sw), ("db3", sg + sh), ("dbr", sg)):
        assert torch.equal(a[k], b[k] * 2.0 ** s), k
    assert torch.equal(a["raws"][0], b["raws"][0] * 2.0 ** (sx + sw)) and torch.equal(a["d_feats"][0], b["d_feats"][0] * 2.0 ** (sg + sh + sw))


@pytest.mark.parametrize("scale", list(SCALES))
def test_cpu_preconditions_at_bench_size(scale):
    """The 89 523 positions of an 800 x 1344 frame.  Every conv output's sum of absolute terms is at most 2304 x 4 x 2 + 4 x 4 x 265 < 2^15
    units whatever the data, so the fp32 CPU convolution used here is exact (the premise test shows it on the small sets); the sums over
    positions (head weight gradient, db3, the 3x3 weight gradient through the bound max|x| * sum_p |d_raw|) are taken from the data."""
    d = make_head_case(FPN, scale)
    assert float(bf(d["w3"]).abs().reshape(C_, -1).sum(1).max()) / d["u_w3"] * 4 < 2 ** 15
    st = new_stats()
    raws = []
    for f in d["feats"]:
        acc = conv64(f, bf(d["w3"]), torch.float32)
        raws.append(bf(acc))
        st["raw_big"] += int((acc.abs() > 256 * d["u_raw"]).sum()); st["raw_rounded"] += int((raws[-1] != acc).sum()); st["raw_ties"] += bf16_ties(acc)
    _, _, zs = tail_forward_ref(raws, d, st)
    d_raws = tail_backward_ref(zs, d, st)[0]
    assert st["raw_big"] > 0 and st["raw_ties"] > 0 and st["z_zero"] > 0 and st["h_ties"] > 0 and st["dz_masked_at_zero"] > 0, st
    per_co = sum(t.abs().reshape(C_, -1).sum(1) for t in d_raws)
    assert float(per_co.max()) / d["u_dz"] * 4 < LIMIT                       # |dW3[co, ci, tap]| terms: sum_p |d_raw[co, p]| * max |x|
    assert float(torch.cat([t.abs().flatten() for t in d_raws]).max()) / d["u_dz"] * float(bf(d["w3"]).abs().sum((0, 2, 3)).max()) / d["u_w3"] < LIMIT


# ------------------------------------------------------------------------------------------ the fused head (csrc/rpn_conv.hip)
@pytest.fixture(scope="module")
def ops():
    from faster_rcnn_pytorch_amd import ops as o
    return o


def _dev32(t):
    return t.float().to(DEV)


def _devbf(t):
    return t.float().bfloat16().to(DEV)


def _run_head(ops, d):
    fin = [_devbf(f).requires_grad_(True) for f in d["feats"]]
    params = [_dev32(d[k]).requires_grad_(True) for k in ("w3", "b3")] + [_dev32(d["wc"]).reshape(2 * A, C_, 1, 1).requires_grad_(True), _dev32(d["bc"]).requires_grad_(True),
                                                                       _dev32(d["wr"]).reshape(4 * A, C_, 1, 1).requires_grad_(True), _dev32(d["br"]).requires_grad_(True)]
    cls, reg = ops.rpn_conv_head_levels(fin, *params)
    raws = [t.detach().clone() for t in cls.grad_fn.saved_tensors[4 + len(fin):]]       # the stored bf16 planes of the bias-free 3x3 output
    torch.autograd.backward([cls, reg], [_dev32(d["gc"]), _dev32(d["gr"])])
    return {"cls": cls.detach(), "reg": reg.detach(), "raws": raws, "d_feats": [f.grad for f in fin], "dw3": params[0].grad, "db3": params[1].grad,
            "dwc": params[2].grad.reshape(2 * A, C_), "dbc": params[3].grad, "dwr": params[4].grad.reshape(4 * A, C_), "dbr": params[5].grad}


def _compare_head(got, ref, keys=("cls", "reg", "dw3", "db3", "dwc", "dbc", "dwr", "dbr")):
    for k in keys:
        same_bits(got[k], ref[k], k)
    for lk in ("raws", "d_feats"):
        for i, (a, b) in enumerate(zip(got[lk], ref[lk])):
            assert a.dtype == torch.bfloat16
            same_bits(a, b, "%s[%d]" % (lk, i))


@gpu
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("name", list(SHAPE_SETS))
def test_rpn_conv_head_levels_forward_and_backward_bit_for_bit(ops, name, scale):
    """ops.rpn_conv_head_levels: cls, reg, the stored raw planes; bf16 data gradients per level, dW3, db3, dWc, dbc, dWr, dbr."""
    d = make_head_case(SHAPE_SETS[name], scale)
    ref = head_reference(d, DEV)
    assert_not_vacuous(ref["stats"])
    assert ref["stats"]["dz_masked_at_zero"] > 0               # a `>=` in the backward's ReLU mask would let these gradients through
    got = _run_head(ops, d)
    assert got["cls"].dtype == got["dw3"].dtype == got["db3"].dtype == torch.float32
    _compare_head(got, ref)
    again = _run_head(ops, d)                                  # stale workspace, per-call state
    for k in ("cls", "reg", "dw3", "db3", "dwc", "dbc", "dwr", "dbr"):
        assert torch.equal(got[k], again[k]), k
    for lk in ("raws", "d_feats"):
        assert all(torch.equal(a, b) for a, b in zip(got[lk], again[lk])), lk


@gpu
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("name", list(SHAPE_SETS))
def test_rpn_conv_bwd_data_and_wgrad_on_their_own_bit_for_bit(ops, name, scale):
    """ops.rpn_conv_bwd_data and ops.rpn_conv_wgrad with upstream gradients of their own in [-2, 2] (the issue's worst case for the weight
    gradient: 89 523 x 4 x 2 = 716 184 units), and wide d_raw values (> 256 units) so that the data gradient's rounding is exercised."""
    sx, sw, _, sg = SCALES[scale]
    shapes = SHAPE_SETS[name]
    gen = torch.Generator().manual_seed(77)
    feats = [dyadic(gen, (1, C_, h, w), -4, 4, sx) for h, w in shapes]
    d_raws = [dyadic(gen, (1, C_, h, w), -2, 2, sg) for h, w in shapes]
    d_wide = [bf(dyadic(gen, (1, C_, h, w), -40, 40, sg)) for h, w in shapes]
    w3 = plant_wide(gen, dyadic(gen, (C_, C_, 3, 3), -2, 2), range(3, C_, 8), 4) * 2.0 ** -sw
    st = {}
    ref_w = wgrad_ref([f.to(DEV) for f in feats], [t.to(DEV) for t in d_raws], 2.0 ** -(sx + sg), st)
    ref_d = bwd_data_ref([t.to(DEV) for t in d_wide], w3.to(DEV), 2.0 ** -(sw + sg), st)
    assert st["dx_rounded"] > 0 and st["dx_ties"] > 0 and int((bf(w3) != w3).sum()) > 0, st
    for rep in range(2):
        got_w = ops.rpn_conv_wgrad([_devbf(f) for f in feats], [_devbf(t) for t in d_raws])
        got_d = ops.rpn_conv_bwd_data([_devbf(t) for t in d_wide], _dev32(w3))
        assert got_w.dtype == torch.float32
        same_bits(got_w, ref_w, "dW3 (call %d)" % rep)
        for i, (a, b) in enumerate(zip(got_d, ref_d)):
            assert a.dtype == torch.bfloat16
            same_bits(a, b, "d_x[%d] (call %d)" % (i, rep))


# ------------------------------------------------------------------------------------------ the tail kernels' bf16 form (csrc/rpn_head.hip)
@gpu
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("name", ["fpn800x1344", "tiny", "smallest_first", "twins"])
def test_rpn_head_tail_bf16_forward_and_backward_bit_for_bit(ops, name, scale):
    """ops.rpn_head_tail_levels(mfma="bf16") on bf16 raw inputs: cls, reg, d_raw, the head gradients and db3."""
    d = make_head_case(SHAPE_SETS[name], scale, seed=1)
    gen = torch.Generator().manual_seed(5)
    raws = [bf(dyadic(gen, (1, C_, h, w), -300, 300, 0)) * d["u_raw"] for h, w in SHAPE_SETS[name]]
    dd = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items() if k != "feats"}
    st = new_stats()
    cls, reg, zs = tail_forward_ref([r.to(DEV) for r in raws], dd, st)
    d_raws, dwc, dbc, dwr, dbr, db3 = tail_backward_ref(zs, dd, st)
    assert st["h_rounded"] > 0 and st["h_ties"] > 0 and st["z_zero"] > 0 and st["dz_masked_at_zero"] > 0, st
    prev = None
    for rep in range(2):
        rin = [_devbf(r).requires_grad_(True) for r in raws]
        params = [_dev32(d["b3"]), _dev32(d["wc"]).reshape(2 * A, C_, 1, 1), _dev32(d["bc"]), _dev32(d["wr"]).reshape(4 * A, C_, 1, 1), _dev32(d["br"])]
        params = [p.requires_grad_(True) for p in params]
        gc_, gr_ = ops.rpn_head_tail_levels(rin, *params, mfma="bf16")
        torch.autograd.backward([gc_, gr_], [_dev32(d["gc"]), _dev32(d["gr"])])
        got = [gc_.detach(), gr_.detach(), params[0].grad, params[1].grad.reshape(2 * A, C_), params[2].grad, params[3].grad.reshape(4 * A, C_), params[4].grad]
        for a, b, k in zip(got, (cls, reg, db3, dwc, dbc, dwr, dbr), ("cls", "reg", "db3", "dwc", "dbc", "dwr", "dbr")):
            assert a.dtype == torch.float32
            same_bits(a, b, k)
        for i, (a, b) in enumerate(zip(rin, d_raws)):
            assert a.grad.dtype == torch.bfloat16
            same_bits(a.grad, b, "d_raw[%d]" % i)
        if prev is not None:
            assert all(torch.equal(a, b) for a, b in zip(got + [r.grad for r in rin], prev))
        prev = got + [r.grad for r in rin]


# ------------------------------------------------------------------------------------------ ops.conv3x3_bf16_c256
@gpu
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("hw", [(100, 168), (200, 336), (103, 165)])
def test_conv3x3_bf16_c256_forward_and_backward_bit_for_bit(ops, hw, with_bias, scale):
    """The FPN's output convolution: y = bf16(bf16(conv(x, bf16(W))) + bf16(bias)) -- the bias joins AFTER the rounding, in bf16 --,
    dx = bf16(conv_transpose(g, bf16(W))), dW fp32, db = bf16(sum of g) (autograd's, through the bf16 bias cast)."""
    sx, sw, _, sg = SCALES[scale]
    gen = torch.Generator().manual_seed(hw[0] + 3 * with_bias)
    x = dyadic(gen, (1, C_, *hw), -4, 4, sx)
    w = plant_wide(gen, dyadic(gen, (C_, C_, 3, 3), -2, 2), range(3, C_, 8), 4) * 2.0 ** -sw
    b = dyadic(gen, (C_,), -4, 4, sx + sw) if with_bias else None
    g = dyadic(gen, (1, C_, *hw), -2, 2, sg, keep=0.5)
    u = 2.0 ** -(sx + sw)
    xd, wr, gd = x.to(DEV), bf(w).to(DEV), g.to(DEV)
    acc = conv64(xd, wr)
    need_exact(conv64(xd.abs(), wr.abs()), u, "y")
    y_ref = bf(acc)
    need_normal(y_ref, "y")
    assert int((acc.abs() > 256 * u).sum()) > 0 and int((y_ref != acc).sum()) > 0 and bf16_ties(acc) > 0
    if with_bias:
        s = y_ref + bf(b).to(DEV).view(1, -1, 1, 1)
        y_ref = bf(s)
        assert int((y_ref != s).sum()) > 0                     # the second rounding happens
    dx_ref = bwd_data_ref([gd], w.to(DEV), 2.0 ** -(sw + sg))[0]
    dw_ref = wgrad_ref([xd], [gd], 2.0 ** -(sx + sg), {})
    db_ref = bf(gd.sum((0, 2, 3)))                             # autograd sums the bf16 gradient of the bf16 bias cast: fp32 accumulation, one rounding
    need_exact(gd.abs().sum((0, 2, 3)), 2.0 ** -sg, "db")
    prev = None
    for rep in range(2):
        xi, wi = _devbf(x).requires_grad_(True), _dev32(w).requires_grad_(True)
        bi = _dev32(b).requires_grad_(True) if with_bias else None
        y = ops.conv3x3_bf16_c256(xi, wi, bi)
        y.backward(_devbf(g))
        assert y.dtype == xi.grad.dtype == torch.bfloat16 and wi.grad.dtype == torch.float32
        same_bits(y.detach(), y_ref, "y"); same_bits(xi.grad, dx_ref, "dx"); same_bits(wi.grad, dw_ref, "dW")
        got = [y.detach(), xi.grad, wi.grad]
        if with_bias:
            same_bits(bi.grad, db_ref, "db")
            got.append(bi.grad)
        if prev is not None:
            assert all(torch.equal(a, c) for a, c in zip(got, prev))
        prev = got


# ------------------------------------------------------------------------------------------ known answers: impulse, NaN footprint
IMPULSE_LEVELS = [(17, 65), (9, 33)]                                   # level 0: 3 x 3 tiles of 8 x 32, the last one a single odd column
IMPULSES = {"tile_corner_top_left": (0, 8, 32), "tile_corner_top_right": (0, 8, 63), "tile_corner_bottom_left": (0, 15, 32), "tile_corner_bottom_right": (0, 15, 63),
            "map_corner_top_left": (0, 0, 0), "map_corner_top_right": (0, 0, 64), "map_corner_bottom_left": (0, 16, 0), "map_corner_bottom_right": (0, 16, 64),
            "last_column_of_odd_width": (0, 7, 64), "first_pixel_of_second_level": (1, 0, 0)}


def _placed(w, ch_axis, ch, hw, py, px, amp):
    """The expected map of a 3 x 3 / pad 1 correlation of an impulse `amp` at (py, px) of channel ch: out[:, py + 1 - ky, px + 1 - kx] = amp * w[.., ky, kx]."""
    out = torch.zeros(1, C_, *hw, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            yy, xx = py + 1 - ky, px + 1 - kx
            if 0 <= yy < hw[0] and 0 <= xx < hw[1]:
                out[0, :, yy, xx] = amp * (w[:, ch, ky, kx] if ch_axis == 1 else w[ch, :, 2 - ky, 2 - kx])
    return out


@gpu
@pytest.mark.parametrize("where", list(IMPULSES))
def test_impulse_gives_the_flipped_weight_slice_there_and_zero_elsewhere(ops, where):
    """One nonzero input pixel: the output is the weight slice around it and zero elsewhere -- a failure names the seam.  Checked for the
    fused head (raw, and cls / reg from that raw), the data-gradient kernel and conv3x3_bf16_c256."""
    lvl, py, px = IMPULSES[where]
    ch = (37 * (1 + list(IMPULSES).index(where))) % C_
    d = make_head_case(IMPULSE_LEVELS, "s0", seed=2)
    d["w3"] = dyadic(torch.Generator().manual_seed(9), (C_, C_, 3, 3), -3, 3)          # no wide entries: the slice itself must come back
    d["feats"] = [torch.zeros(1, C_, h, w, dtype=torch.float64) for h, w in IMPULSE_LEVELS]
    d["feats"][lvl][0, ch, py, px] = 3.0
    want = [torch.zeros(1, C_, h, w, dtype=torch.float64) for h, w in IMPULSE_LEVELS]
    want[lvl] = _placed(d["w3"], 1, ch, IMPULSE_LEVELS[lvl], py, px, 3.0)
    assert torch.equal(want[lvl], F.conv2d(d["feats"][lvl], d["w3"], None, padding=1))
    dd = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items() if k != "feats"}
    cls_ref, reg_ref, _ = tail_forward_ref([t.to(DEV) for t in want], dd, new_stats())
    for rep in range(2):
        got = _run_head(ops, d)
        for i in range(2):
            same_bits(got["raws"][i], want[i], "raw[%d]" % i)
        same_bits(got["cls"], cls_ref, "cls"); same_bits(got["reg"], reg_ref, "reg")
        # the data gradient: an impulse in d_raw's channel ch comes back as w3[ch, :, flipped taps]
        dx = ops.rpn_conv_bwd_data([_devbf(f) for f in d["feats"]], _dev32(d["w3"]))
        want_dx = _placed(d["w3"], 0, ch, IMPULSE_LEVELS[lvl], py, px, 3.0)
        assert torch.equal(want_dx, F.conv_transpose2d(d["feats"][lvl], d["w3"], padding=1))
        for i in range(2):
            same_bits(dx[i], want_dx if i == lvl else torch.zeros_like(want[i]), "d_x[%d]" % i)
        y = ops.conv3x3_bf16_c256(_devbf(d["feats"][lvl]), _dev32(d["w3"]))
        same_bits(y, want[lvl], "conv3x3_bf16_c256")


@gpu
@pytest.mark.parametrize("lvl,py,px", [(0, 8, 32), (0, 16, 64), (1, 0, 0)], ids=["tile_corner", "map_corner_odd_column", "second_level_first_pixel"])
def test_nan_footprint_is_the_3x3_neighbourhood_and_nothing_else(ops, lvl, py, px):
    """One NaN input pixel in one channel (ordinary data): raw / y are NaN at exactly the 3 x 3 neighbourhood inside the map for every
    output channel and cls / reg at exactly those positions; every other element has the bits of the NaN-free run.  A kernel that reads a
    neighbour it should not (or a stale LDS pixel) and multiplies it by a zero weight passes every finite test and fails here; so does a
    fused ReLU that turns a NaN into 0."""
    d = make_head_case(IMPULSE_LEVELS, "real", seed=3)
    clean = _run_head(ops, d)
    d["feats"][lvl][0, 5, py, px] = float("nan")
    got = _run_head(ops, d)
    hh, ww = IMPULSE_LEVELS[lvl]
    foot = torch.zeros(hh, ww, dtype=torch.bool)
    foot[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
    foot = foot.to(DEV)
    for i in range(2):
        nan = torch.isnan(got["raws"][i])
        want = foot[None, None].expand(1, C_, hh, ww) if i == lvl else torch.zeros_like(nan)
        assert torch.equal(nan, want), "raw[%d]: NaN at %d elements, expected %d" % (i, int(nan.sum()), int(want.sum()))
        assert torch.equal(got["raws"][i].view(torch.int16)[~nan], clean["raws"][i].view(torch.int16)[~nan])
    p0 = sum(h * w for h, w in IMPULSE_LEVELS[:lvl])
    pos = torch.zeros(sum(h * w for h, w in IMPULSE_LEVELS), dtype=torch.bool, device=DEV)
    pos[p0:p0 + hh * ww] = foot.flatten()
    for k, n in (("cls", 2 * A), ("reg", 4 * A)):
        nan = torch.isnan(got[k]).reshape(-1, n)
        assert torch.equal(nan, pos[:, None].expand(-1, n)), "%s: NaN at %d elements, expected %d" % (k, int(nan.sum()), int(pos.sum()) * n)
        assert torch.equal(got[k].reshape(-1, n)[~pos].view(torch.int32), clean[k].reshape(-1, n)[~pos].view(torch.int32))
    # the plain convolution (with its bias) and the tail's bf16 form on the head's own raw
    b = _dev32(d["b3"])
    y0 = ops.conv3x3_bf16_c256(_devbf(torch.nan_to_num(d["feats"][lvl], nan=1.0)), _dev32(d["w3"]), b)
    y = ops.conv3x3_bf16_c256(_devbf(d["feats"][lvl]), _dev32(d["w3"]), b)
    nan = torch.isnan(y)
    assert torch.equal(nan, foot[None, None].expand(1, C_, hh, ww))
    assert torch.equal(y.view(torch.int16)[~foot[None, None].expand_as(y)], y0.view(torch.int16)[~foot[None, None].expand_as(y)])
    c2, r2 = ops.rpn_head_tail_levels(got["raws"], b, _dev32(d["wc"]).reshape(2 * A, C_, 1, 1), _dev32(d["bc"]), _dev32(d["wr"]).reshape(4 * A, C_, 1, 1), _dev32(d["br"]),
                                      mfma="bf16")
    assert torch.equal(torch.isnan(c2), torch.isnan(got["cls"])) and torch.equal(torch.isnan(r2), torch.isnan(got["reg"]))
    assert torch.equal(torch.nan_to_num(c2, nan=7.0), torch.nan_to_num(got["cls"], nan=7.0)) and torch.equal(torch.nan_to_num(r2, nan=7.0), torch.nan_to_num(got["reg"], nan=7.0))


# ------------------------------------------------------------------------------------------ affine_act_mixed at zero, NaN, -inf
@gpu
@pytest.mark.parametrize("form", ["inner", "stream", "stream_res_twin", "f32_res_twin"])
def test_affine_act_mixed_at_exact_zero_nan_and_minus_infinity(ops, form):
    """The four forms of test_affine_act_mixed_is_the_autocast_torch_form with pre-activations equal to exactly zero (values and
    gradients, bit for bit with autograd on the torch form: the mask is `> 0`), and a NaN / -inf activation through the fused ReLU as
    through torch.relu (forward)."""
    g = torch.Generator().manual_seed(12)
    C2, H, W = 64, 29, 45
    xb = (form != "f32_res_twin")
    with_res, twin, inner = form.endswith("res_twin"), form.endswith("twin"), form == "inner"
    x = torch.randint(-4, 5, (1, C2, H, W), generator=g).float().to(DEV)            # integers: x * scale + shift (+ res) hits zero exactly, often
    scale = torch.randint(1, 3, (C2,), generator=g).float().to(DEV)
    shift = torch.randint(-4, 5, (C2,), generator=g).float().to(DEV)
    r0 = torch.randint(-2, 3, (1, C2, H, W), generator=g).float().to(DEV) if with_res else None

    def torch_form(x_, r_):
        y32 = x_.float() * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)
        if with_res:
            y32 = y32 + r_
        y32 = torch.relu(y32)
        return (y32.bfloat16() if inner else y32), (y32.bfloat16() if twin else None), y32

    def lib_form(x_, r_):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = ops.affine_act_mixed(x_, scale, shift, r_, relu=True, out_bf16=inner, twin=twin)
        return out if twin else (out, None)
    x = (x.bfloat16() if xb else x).requires_grad_(True)
    r = r0.clone().requires_grad_(True) if with_res else None
    pre = x.detach().float() * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1) + (r0 if with_res else 0)
    assert int((pre == 0).sum()) > 100
    dy = torch.randint(-3, 4, (1, C2, H, W), generator=g).float().to(DEV)
    dy = dy.bfloat16() if inner else dy
    dt = torch.randint(-3, 4, (1, C2, H, W), generator=g).float().to(DEV).bfloat16() if twin else None
    ref, ref_twin, _ = torch_form(x, r)
    torch.autograd.backward([ref] + ([ref_twin] if twin else []), [dy] + ([dt] if twin else []))
    want = [x.grad.clone()] + ([r.grad.clone()] if with_res else [])
    x.grad = None
    if with_res:
        r.grad = None
    y, yt = lib_form(x, r)
    assert torch.equal(y, ref) and (not twin or torch.equal(yt, ref_twin))
    torch.autograd.backward([y] + ([yt] if twin else []), [dy] + ([dt] if twin else []))
    for a_, c_ in zip([x.grad] + ([r.grad] if with_res else []), want):
        assert a_.dtype == c_.dtype and torch.equal(a_, c_)
    assert bool((x.grad[pre == 0] == 0).all())                                       # nothing flows through a pre-activation of exactly zero
    xn = x.detach().clone()
    xn[0, 3, 5, 7] = float("nan")
    xn[0, 4, 0, 0] = float("-inf")
    xn[0, 4, 28, 44] = float("inf")
    yn, ytn = lib_form(xn, r0)
    rn, rtn, _ = torch_form(xn, r0)
    assert bool(torch.isnan(yn[0, 3, 5, 7])) and int(torch.isnan(yn).sum()) == 1 and float(yn[0, 4, 0, 0]) == 0.0 and float(yn[0, 4, 28, 44]) == float("inf")
    assert torch.equal(torch.isnan(yn), torch.isnan(rn)) and torch.equal(torch.nan_to_num(yn.float(), nan=7.0), torch.nan_to_num(rn.float(), nan=7.0))
    if twin:
        assert torch.equal(torch.isnan(ytn), torch.isnan(rtn)) and torch.equal(torch.nan_to_num(ytn.float(), nan=7.0), torch.nan_to_num(rtn.float(), nan=7.0))
