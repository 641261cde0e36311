"""CPU-only: the fp32 conv stage's host rules through ops.conv3x3_plan (frcnn_conv3x3_f32_plan: the functions the launches use, nothing launched; without a
device the stage assumes 256 CUs).  Every case of tests/conv_plan_cases.py is in the plan class it names, the table as a whole covers every value of every
plan field the rules can reach, what they cannot reach is named with the reason, `supported` implies a plan within the control block's limits, and the cases
of the older tests are in the classes their comments claim."""
import itertools
import os

import pytest

from conv_plan_cases import CASES, UNREACHABLE, get

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CF_MAX_TILES = 32768                                                  # csrc/rpn_conv_f32.hip: ticket words in the control block


@pytest.fixture(scope="module")
def ops():
    so = os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import ops as o
    if o.conv3x3_plan([(8, 8)], 64, 64)["G"] != 512:
        pytest.skip("the expectations are written for 256 CUs (G = 512); this host has a device with %d slots" % o.conv3x3_plan([(8, 8)], 64, 64)["G"])
    return o


def _supported(ops, shapes, Cin, Cout, grads):
    H, W = ops._host_i32([h for h, _ in shapes]), ops._host_i32([w for _, w in shapes])
    return bool(ops.lib.frcnn_conv3x3_f32_supported(ops._np_ptr(H), ops._np_ptr(W), len(shapes), Cin, Cout, 1 if grads else 0))


@pytest.fixture(scope="module")
def plans(ops):
    return {c.name: ops.conv3x3_plan(c.shapes, c.Cin, c.Cout) for c in CASES}


def test_case_names_are_unique_and_the_table_is_well_formed():
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        assert c.act in ("none", "relu", "pool") and c.expect and c.cls
        assert c.Cout % 64 == 0 and c.Cin % 32 == 0 and (c.Cin % 64 == 0) == c.grads, c.name      # forward-only exactly where the gradients cannot run
        assert min(c.Cin, c.Cout) == 64 or "rows" in c.name or "fwd_only" in c.name, c.name       # the smaller side 64 unless the class is about the channel side
        for h, w in c.shapes:
            assert (h <= 141 and w <= 141) or h <= 40, c.name          # small maps; the wide-strip cases a few tile rows high


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_is_in_the_class_it_names(plans, case):
    p = plans[case.name]
    for path, want in case.expect.items():
        assert get(p, path) == want, (case.name, path, get(p, path), want, p)
    if case.act == "pool":
        assert p["pool"], case.name
    assert (p["bwd_data"] is not None) == case.grads and (p["wgrad"] is not None) == case.grads


def _products(p):
    return [(k, p[k]) for k in ("fwd", "bwd_data") if p[k] is not None]


def test_table_covers_every_reachable_value_of_every_plan_field(plans):
    P = [(c, plans[c.name]) for c in CASES]
    have = lambda pred: [c.name for c, p in P if pred(c, p)]            # noqa: E731
    missing = []

    def need(what, pred):
        if not have(pred):
            missing.append(what)
    # tile size x padding; product tile width follows the padding
    for m, tg in itertools.product((2, 4), (64, 128)):
        need("F(%dx%d) padded to %d" % (m, m, tg), lambda c, p: p["tile"] == m and p["tg"] == tg and p["fwd"]["tile_w"] == tg)
    # every schedule on every product tile height, both tile sizes (forward or data gradient)
    for m, th, s in itertools.product((2, 4), (64, 128), ("stream_k", "whole_ranges", "one_tile")):
        need("F(%dx%d) %d-row %s" % (m, m, th, s), lambda c, p: p["tile"] == m and any(d["tile_h"] == th and d["schedule"] == s for _, d in _products(p)))
    for k in ("fwd", "bwd_data"):
        for tg in (64, 128):
            need("fused_out64 %s tg %d" % (k, tg), lambda c, p: p[k] is not None and p[k]["schedule"] == "fused_out64" and p["tg"] == tg and p["tile"] == 4)
        for th in (64, 128):
            need("%s %d-row with several tiles along the channel side" % (k, th), lambda c, p: p[k] is not None and p[k]["tile_h"] == th and p[k]["m_tiles"] > 1)
    # the weight gradient's four tile shapes, several tiles along either 64-wide side
    for th, tw in itertools.product((64, 128), (64, 128)):
        need("wgrad %d x %d" % (th, tw), lambda c, p: p["wgrad"] is not None and (p["wgrad"]["tile_h"], p["wgrad"]["tile_w"]) == (th, tw))
    need("wgrad 64-row mt > 1", lambda c, p: p["wgrad"] is not None and p["wgrad"]["tile_h"] == 64 and p["wgrad"]["m_tiles"] > 1)
    need("wgrad NW = 64 nt > 1", lambda c, p: p["wgrad"] is not None and p["wgrad"]["tile_w"] == 64 and p["wgrad"]["t_tiles"] > 1)
    need("wgrad 64 x 64 mt > 1 and nt > 1", lambda c, p: p["wgrad"] is not None and p["wgrad"]["tile_h"] == p["wgrad"]["tile_w"] == 64
         and p["wgrad"]["m_tiles"] > 1 and p["wgrad"]["t_tiles"] > 1)
    # strips and segments
    for m in (2, 4):
        lv = lambda p: p["strips_in"]["levels"]                         # noqa: E731
        need("F(%dx%d) one segment" % (m, m), lambda c, p: p["tile"] == m and all(l["segments"] == 1 for l in lv(p)))
        need("F(%dx%d) two segments" % (m, m), lambda c, p: p["tile"] == m and any(l["segments"] == 2 for l in lv(p)))
        need("F(%dx%d) last segment of one tile" % (m, m), lambda c, p: p["tile"] == m and any(l["segments"] == 2 and l["last_segment_tiles"] == 1 for l in lv(p)))
        need("F(%dx%d) several strips in a level, the last one partial" % (m, m), lambda c, p: p["tile"] == m and any(
            l["last_strip_rows"] and -(-h // m) > l["rows"] for l, (h, _) in zip(lv(p), c.shapes)))
        need("F(%dx%d) several strips in a level, the last one full" % (m, m), lambda c, p: p["tile"] == m and any(
            not l["last_strip_rows"] and -(-h // m) > l["rows"] for l, (h, _) in zip(lv(p), c.shapes)))
        for pb in ((1024, 512, 256) if m == 2 else (512, 256)):
            need("F(%dx%d) per_block %d" % (m, m, pb), lambda c, p: p["tile"] == m and pb in (p["strips_in"]["per_block"], p["strips_out"]["per_block"]))
    # levels, activations, forward-only widths
    need("8 levels with several 1 x 1", lambda c, p: len(c.shapes) == 8 and sum(s == (1, 1) for s in c.shapes) >= 3)
    need("8 levels on F(4x4)", lambda c, p: len(c.shapes) == 8 and p["tile"] == 4)
    for tg in (64, 128):
        need("pool, tg %d, unfused product" % tg, lambda c, p: c.act == "pool" and p["tg"] == tg and p["fwd"]["schedule"] != "fused_out64")
    need("pool, tg 64, fused product", lambda c, p: c.act == "pool" and p["tg"] == 64 and p["fwd"]["schedule"] == "fused_out64")
    for cin in (32, 96, 160):
        need("forward only, Cin = %d" % cin, lambda c, p: c.Cin == cin and not c.grads and p["fwd"]["Kc"] == cin // 32)
    for act, bias in itertools.product(("none", "relu", "pool"), (False, True)):
        need("act %s bias %s" % (act, bias), lambda c, p: c.act == act and c.bias == bias)
    # schedule boundaries at G = 512
    G = 512
    for n, s in ((G, "one_tile"), (3 * G // 4, "one_tile"), (2 * G, "whole_ranges"), (1008, "stream_k"), (1080, "stream_k")):
        need("n_tiles = %d: %s" % (n, s), lambda c, p: any(d["n_tiles"] == n and d["schedule"] == s for _, d in _products(p)))
    need("stream-K at n_tiles >= 2 G", lambda c, p: any(d["n_tiles"] >= 2 * G and d["schedule"] == "stream_k" for _, d in _products(p)))
    need("stream-K below 3/4 G with fewer units than slots", lambda c, p: any(d["schedule"] == "stream_k" and d["G"] < G for _, d in _products(p)))
    for th in (64, 128):
        need("G .. 2 G band on the %d-row tile" % th, lambda c, p: any(G < d["n_tiles"] < 2 * G and d["tile_h"] == th and d["schedule"] == "stream_k" for _, d in _products(p)))
    assert not missing, missing


def test_unreachable_classes_are_named_with_a_reason_and_nothing_lands_in_them(ops, plans):
    assert all(len(why) > 40 for why in UNREACHABLE.values())
    seen = list(plans.values())
    for h, w, n, (ci, co) in itertools.product((1, 5, 24, 33, 64, 100), (1, 7, 40, 130, 300, 700), (1, 3, 8), ((64, 64), (64, 512), (256, 128))):
        shapes = [(h, w)] + [(max(1, h // (l + 1)), max(1, w // (2 * l + 1))) for l in range(1, n)]
        if _supported(ops, shapes, ci, co, True):
            seen.append(ops.conv3x3_plan(shapes, ci, co))
    assert len(seen) > 150
    for p in seen:
        for s in ("strips_in", "strips_out"):
            assert p[s]["per_block"] in ((1024, 512, 256) if p["tile"] == 2 else (512, 256)), p
        assert p["wgrad"] is None or p["wgrad"]["schedule"] == "stream_k"
        assert p["pool"] == (p["tile"] == 4)
        for _, d in _products(p):
            assert d["schedule"] != "fused_out64" or p["tile"] == 4


def test_supported_implies_a_plan_within_the_control_blocks_limits(ops):
    """A grid of small shapes, one to three levels, every channel multiple the stage takes: where frcnn_conv3x3_f32_supported says yes, the plan query
    succeeds and every product stays within the ticket words and the 31-bit unit count; where it says no for the forward, the query refuses."""
    from faster_rcnn_pytorch_amd._lib import FrcnnError
    sizes = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 64, 65, 129, 257, 513, 1025)
    chans = (32, 64, 96, 128, 192, 320, 512, 1024, 4096)
    n_yes = n_no = 0
    for (h, w), ci, co in itertools.product(itertools.product(sizes, sizes), chans, chans):
        for shapes in ([(h, w)], [(h, w), (w, h), (1, 1)]):
            fwd, grads = _supported(ops, shapes, ci, co, False), _supported(ops, shapes, ci, co, True)
            if not fwd:
                n_no += 1
                assert not grads
                with pytest.raises(FrcnnError):
                    ops.conv3x3_plan(shapes, ci, co)
                continue
            n_yes += 1
            p = ops.conv3x3_plan(shapes, ci, co)
            assert (p["bwd_data"] is not None) == grads == (p["wgrad"] is not None)
            for k in ("fwd", "bwd_data", "wgrad"):
                d = p[k]
                if d is None:
                    continue
                assert 0 < d["n_tiles"] <= CF_MAX_TILES and 0 < d["units"] < 2 ** 31 and d["units"] == d["n_tiles"] * d["Kc"], (shapes, ci, co, k, d)
                assert 0 < d["G"] <= (p["G_wgrad"] if k == "wgrad" else p["G"]) and d["G"] <= d["units"]
                assert d["n_tiles"] == (p["tile"] + 2) ** 2 * d["m_tiles"] * d["t_tiles"]
                if d["schedule"] == "one_tile":
                    assert d["G"] == d["n_tiles"]
                if d["schedule"] == "whole_ranges":
                    assert d["n_tiles"] >= 2 * d["G"]
            assert p["padded_tiles"] % p["tg"] == 0 and p["fwd"]["t_tiles"] * p["tg"] == p["padded_tiles"]
    assert n_yes > 10000 and n_no > 1000


def test_the_older_tests_cases_are_in_the_classes_their_comments_claim(ops):
    import test_gpu_conv_merged_launches as ml
    import test_gpu_ops as tg
    by = {c[0]: ops.conv3x3_plan(c[3], c[1], c[2]) for c in tg.CONV3X3_CASES + tg.SPLIT_CASES}
    p = by["vgg_conv1_2"]                                               # "64-wide tiles on both sides (F(4x4): 1500 tiles)"
    assert p["tile"] == 4 and p["padded_tiles"] == 1536 and p["fwd"]["schedule"] == "fused_out64" and (p["wgrad"]["tile_h"], p["wgrad"]["tile_w"]) == (64, 64)
    assert by["vgg_conv2_1"]["bwd_data"]["tile_h"] == 64 and by["vgg_conv2_1"]["fwd"]["tile_h"] == 128        # "a 64-channel input side"
    assert by["narrow_both"]["tile"] == 2 and by["narrow_both"]["fwd"]["tile_h"] == 64                       # "the same with F(2x2)"
    assert by["wide_out_64"]["fwd"]["tile_h"] == 64 and by["wide_out_64"]["fwd"]["m_tiles"] == 1             # "64 outputs of a wide input"
    p = by["rpn_37x62"]                                                 # "160 4 x 4 tiles padded to 192 (64-wide product tiles)"
    assert (p["tile"], p["tg"], p["padded_tiles"], p["fwd"]["tile_w"]) == (4, 64, 192, 64)
    p = by["c5_25x42"]                                                  # "273 2 x 2 tiles padded to 320: the 64-wide product tile with F(2x2)"
    assert (p["tile"], p["tg"], p["padded_tiles"], p["fwd"]["tile_w"]) == (2, 64, 320, 64)
    for name in ("vgg_conv1_2_full", "resnet_layer1_full"):             # the fused 64 -> 64 product, forward and data gradient; 64 x 64 weight-gradient tiles
        p = by[name]
        assert p["fwd"]["schedule"] == p["bwd_data"]["schedule"] == "fused_out64" and (p["wgrad"]["tile_h"], p["wgrad"]["tile_w"]) == (64, 64)
    assert by["vgg_conv1_2_full"]["strips_in"]["levels"][0]["segments"] == 2 and by["vgg_conv1_2_full"]["strips_in"]["levels"][0]["last_segment_tiles"] == 122
    assert all(p["tg"] == 64 or p["tile"] == 4 for p in by.values())    # no F(2x2) case of those tests is padded to 128: what conv_plan_cases adds
    want = {"many_64-128_244x244": ("stream_k", 1080), "whole_128-128_276x276": ("whole_ranges", 1368), "streamk_256-256_40x52": ("stream_k", 216),
            "onetile_512-512_37x62": ("one_tile", 432)}
    for name, (Cin, Cout, hw) in ml.BWD_LAYERS.items():                # "one shape per scheduling mode of the data gradient's product"
        d = ops.conv3x3_plan([hw], Cin, Cout)["bwd_data"]
        assert (d["schedule"], d["n_tiles"]) == want[name], (name, d)
