"""The fp32 conv stage's plan classes, one case each at the smallest shape that reaches it (csrc/rpn_conv_f32.hip: wn_pick_m, wn_padded, wn_product,
wn_wgrad_product, wn_strips; ops.conv3x3_plan reports what they decide).  One table for tests/test_conv_plan_host.py (every case is in the class it names,
at 256 CUs; the table covers every value of every plan field) and tests/test_gpu_conv_plan_seams.py (every case against float64 on the device).

A case: name, Cin, Cout, level shapes, bias, act ("none" | "relu" | "pool"), grads (False: forward only), cls (the class it is there for), expect.
expect: {dotted path into ops.conv3x3_plan's dict: value} at 256 CUs (G = 512 workgroup slots, 256 for the weight gradient), e.g. "fwd.schedule",
"strips_in.levels.0.segments".  Maps stay at or under ~140 x 140 with the smaller channel side 64; the wide-strip cases are a few rows high."""
import collections

Case = collections.namedtuple("Case", "name Cin Cout shapes bias act grads cls expect")

# eight levels of at most 64 2 x 2 tiles each, several of one pixel, sizes in no order: F(2x2), every level padded to 64 -> 512 tiles, 8 product columns of 64
L8_SMALL = [(16, 16), (1, 1), (12, 20), (7, 31), (1, 1), (16, 15), (1, 1), (11, 19)]
# eight levels of 96 .. 112 4 x 4 tiles each: F(4x4), every level padded to 128 -> 1024 tiles
L8_F4 = [(40, 40), (37, 43), (44, 36), (33, 47), (48, 32), (35, 45), (41, 39), (29, 53)]

CASES = [
    # 1. F(2x2) with the tile total padded to 128
    Case("f2_tg128_20x22", 64, 64, [(20, 22)], True, "relu", True, "F(2x2), tiles padded to 128",
         {"tile": 2, "tg": 128, "fwd.tile_h": 64, "fwd.tile_w": 128, "fwd.schedule": "stream_k"}),
    Case("f2_tg128_15x18", 64, 128, [(15, 18)], False, "none", True, "F(2x2), tiles padded to 128, 128-row product tile",
         {"tile": 2, "tg": 128, "fwd.tile_h": 128, "fwd.tile_w": 128, "fwd.schedule": "stream_k", "bwd_data.tile_h": 64}),
    # 2. F(2x2) with more than one strip segment (a tile row wider than 256 tiles)
    Case("f2_two_segments_2x600", 64, 64, [(2, 600)], True, "relu", True, "F(2x2), two strip segments, last one of 44 tiles",
         {"tile": 2, "tg": 64, "strips_in.levels.0.segments": 2, "strips_in.levels.0.last_segment_tiles": 44, "strips_out.levels.0.segments": 2}),
    Case("f2_two_segments_2x514", 64, 64, [(2, 514)], False, "relu", True, "F(2x2), two strip segments, last one of ONE tile",
         {"tile": 2, "strips_in.levels.0.segments": 2, "strips_in.levels.0.last_segment_tiles": 1}),
    Case("f2_wide_levels8_4x514", 64, 64, [(1, 1), (4, 514)] + [(1, 1)] * 6, True, "relu", True,
         "F(2x2) kept by seven one-pixel levels: two segments x two full one-row strips in a level, behind a one-pixel level",
         {"tile": 2, "tg": 64, "padded_tiles": 1024, "strips_in.levels.1.segments": 2, "strips_in.levels.1.rows": 1, "strips_in.levels.1.last_strip_rows": 0,
          "strips_in.n_strips": 11}),
    Case("f2_per_block_512_6x514", 64, 384, [(6, 514)] + [(1, 1)] * 7, True, "relu", True,
         "F(2x2): the output gradient's strips settle on per_block = 512 (two tile rows per strip, the last strip of one); 960 tiles in the G .. 2 G band",
         {"tile": 2, "tg": 64, "strips_out.per_block": 512, "strips_out.levels.0.rows": 2, "strips_out.levels.0.last_strip_rows": 1, "strips_in.per_block": 256,
          "fwd.n_tiles": 960, "fwd.schedule": "stream_k", "fwd.tile_h": 128}),
    # 3. F(4x4) with two segments through the unfused product, a last segment of one tile
    Case("f4_two_segments_3x515", 64, 128, [(3, 515)], True, "relu", True, "F(4x4), two strip segments, last one of ONE tile, unfused product, tiles padded to 64",
         {"tile": 4, "tg": 64, "strips_in.levels.0.segments": 2, "strips_in.levels.0.last_segment_tiles": 1, "fwd.schedule": "stream_k", "fwd.tile_w": 64}),
    Case("f4_two_segments_40x515", 64, 128, [(40, 515)], True, "pool", True, "F(4x4), two strip segments, last one of ONE tile, several strips, one tile per workgroup",
         {"tile": 4, "tg": 128, "strips_in.levels.0.segments": 2, "strips_in.levels.0.last_segment_tiles": 1, "strips_in.n_strips": 10,
          "fwd.schedule": "one_tile", "bwd_data.schedule": "one_tile", "bwd_data.tile_h": 64}),
    # 4. 64-row product tiles with more than one tile along the channel side; the weight gradient's 64-wide side with nt > 1
    Case("rows64_out192_40x40", 64, 192, [(40, 40)], True, "relu", True, "64-row product tiles, 3 along Cout (forward); weight gradient 64 x 64 with mt = 3",
         {"tile": 4, "fwd.tile_h": 64, "fwd.m_tiles": 3, "wgrad.tile_h": 64, "wgrad.m_tiles": 3, "wgrad.tile_w": 64}),
    Case("rows64_in192_40x40", 192, 64, [(40, 40)], True, "none", True, "64-row product tiles, 3 along Cin (data gradient); weight gradient NW = 64 with nt = 3",
         {"tile": 4, "bwd_data.tile_h": 64, "bwd_data.m_tiles": 3, "wgrad.tile_w": 64, "wgrad.t_tiles": 3}),
    Case("rows64_in320_31x34", 320, 64, [(31, 34)], False, "relu", True, "F(2x2): 64-row tiles, 5 along Cin, one tile per workgroup (data gradient); weight gradient nt = 5",
         {"tile": 2, "tg": 64, "bwd_data.tile_h": 64, "bwd_data.m_tiles": 5, "bwd_data.schedule": "one_tile", "bwd_data.n_tiles": 400, "wgrad.t_tiles": 5}),
    Case("rows64_out320_31x34", 64, 320, [(31, 34)], True, "relu", True, "F(2x2): 64-row tiles, 5 along Cout, one tile per workgroup (forward); weight gradient mt = 5",
         {"tile": 2, "tg": 64, "fwd.tile_h": 64, "fwd.m_tiles": 5, "fwd.schedule": "one_tile", "fwd.n_tiles": 400, "wgrad.m_tiles": 5, "wgrad.tile_h": 64}),
    Case("rows64_192_to_320_24x28", 192, 320, [(24, 28)], True, "relu", True, "64-row tiles on both sides: weight gradient 64 x 64 with mt = 5, nt = 3",
         {"fwd.tile_h": 64, "fwd.m_tiles": 5, "bwd_data.tile_h": 64, "bwd_data.m_tiles": 3, "wgrad.tile_h": 64, "wgrad.tile_w": 64, "wgrad.m_tiles": 5, "wgrad.t_tiles": 3}),
    Case("rows128_both_21x24", 128, 256, [(21, 24)], True, "relu", True, "128-row tiles on every side: weight gradient 128 x 128 with mt = 2 (the other corner of the tile shapes)",
         {"tile": 4, "tg": 64, "fwd.tile_h": 128, "bwd_data.tile_h": 128, "wgrad.tile_h": 128, "wgrad.tile_w": 128, "wgrad.m_tiles": 2}),
    # 5. forward-only input widths, Cin % 64 = 32 (ops.conv3x3_supported routes them to the stage under no_grad)
    Case("fwd_only_in32_64x64", 32, 512, [(64, 64)], True, "relu", False, "forward only, Cin = 32: ONE K chunk",
         {"fwd.Kc": 1, "bwd_data": None, "wgrad": None}),
    Case("fwd_only_in96_53x53", 96, 256, [(53, 53)], True, "none", False, "forward only, Cin = 96", {"fwd.Kc": 3, "bwd_data": None, "wgrad": None}),
    Case("fwd_only_in160_41x41", 160, 256, [(41, 41)], False, "relu", False, "forward only, Cin = 160", {"fwd.Kc": 5, "bwd_data": None, "wgrad": None}),
    # 6. FRCNN_MAX_LEVELS levels in one call
    Case("levels8_64_64", 64, 64, [(9, 14), (1, 1), (30, 5), (1, 1), (12, 20), (2, 3), (1, 1), (17, 9)], True, "relu", True,
         "eight levels, three of one pixel, sizes in no order", {"tile": 2, "tg": 64, "padded_tiles": 512, "strips_in.n_strips": 8}),
    Case("levels8_f4_64_512", 64, 512, L8_F4, True, "relu", True, "eight levels on F(4x4); the output gradient's strips settle on per_block = 512",
         {"tile": 4, "tg": 128, "padded_tiles": 1024, "strips_out.per_block": 512, "strips_in.per_block": 256, "fwd.schedule": "stream_k", "fwd.n_tiles": 1152}),
    # 7. the fused 64 -> 64 kernel and the fused ReLU + max-pool with tiles padded to 64
    Case("fused_tg64_33x63", 64, 64, [(33, 63)], True, "relu", True, "fused 64 -> 64 product, tiles padded to 64 (three columns)",
         {"tile": 4, "tg": 64, "padded_tiles": 192, "fwd.schedule": "fused_out64", "bwd_data.schedule": "fused_out64"}),
    Case("fused_tg128_40x44", 64, 64, [(40, 44)], False, "none", True, "fused 64 -> 64 product at the smallest map padded to 128 (one column)",
         {"tile": 4, "tg": 128, "padded_tiles": 128, "fwd.schedule": "fused_out64", "bwd_data.schedule": "fused_out64"}),
    Case("fused_pool_tg64_21x24", 64, 64, [(21, 24)], True, "pool", True, "fused 64 -> 64 product with the fused max-pool, tiles padded to 64 (one column)",
         {"tile": 4, "tg": 64, "padded_tiles": 64, "fwd.schedule": "fused_out64", "pool": True}),
    Case("pool_tg64_33x63", 64, 128, [(33, 63)], True, "pool", True, "fused ReLU + max-pool in the output transform, tiles padded to 64",
         {"tile": 4, "tg": 64, "pool": True, "fwd.schedule": "stream_k", "fwd.tile_w": 64, "fwd.tile_h": 128}),
    Case("pool_tg64_21x24", 64, 128, [(21, 24)], False, "pool", True, "fused ReLU + max-pool, ONE column of 64 tiles",
         {"tile": 4, "tg": 64, "padded_tiles": 64, "pool": True, "fwd.tile_w": 64}),
    # 8. stream-K at n_tiles >= 2 G where the 16 % rule rejects whole-tile ranges
    Case("streamk_above_2G_117x117", 64, 512, [(117, 117)], True, "relu", True, "stream-K at n_tiles = 1152 >= 2 G (whole ranges would cost 33 %)",
         {"tile": 4, "G": 512, "fwd.n_tiles": 1152, "fwd.schedule": "stream_k", "fwd.tile_h": 128, "fwd.G": 512}),
    # 9. the schedule boundaries
    Case("f4_one_tile_432_69x69", 64, 512, [(69, 69)], True, "relu", True, "F(4x4), 128-row: one tile per workgroup at 432 tiles (>= 3/4 G = 384)",
         {"tile": 4, "fwd.n_tiles": 432, "fwd.schedule": "one_tile", "fwd.tile_h": 128, "fwd.G": 432, "bwd_data.schedule": "stream_k"}),
    Case("f4_band_576_77x77", 64, 512, [(77, 77)], False, "none", True, "F(4x4), 128-row: stream-K in the G .. 2 G band (576 tiles)",
         {"tile": 4, "fwd.n_tiles": 576, "fwd.schedule": "stream_k", "fwd.tile_h": 128, "fwd.G": 512}),
    Case("f4_rows64_one_tile_77x77", 192, 64, [(77, 77)], True, "relu", True, "F(4x4), 64-row: one tile per workgroup at 432 tiles (data gradient)",
         {"tile": 4, "bwd_data.n_tiles": 432, "bwd_data.schedule": "one_tile", "bwd_data.tile_h": 64, "bwd_data.G": 432}),
    Case("f4_rows64_band_89x89", 192, 64, [(89, 89)], True, "relu", True, "F(4x4), 64-row: stream-K in the G .. 2 G band (540 tiles, data gradient)",
         {"tile": 4, "bwd_data.n_tiles": 540, "bwd_data.schedule": "stream_k", "bwd_data.tile_h": 64, "bwd_data.G": 512}),
    Case("f4_below_2G_113x113", 64, 512, [(113, 113)], True, "relu", True, "F(4x4): 1008 tiles, just below 2 G = 1024: stream-K",
         {"tile": 4, "fwd.n_tiles": 1008, "fwd.schedule": "stream_k"}),
    Case("f4_above_2G_89x89", 64, 768, [(89, 89)], True, "relu", True, "F(4x4): 1080 tiles, just above 2 G: stream-K (3 tiles per workgroup would cost 42 %)",
         {"tile": 4, "fwd.n_tiles": 1080, "fwd.schedule": "stream_k", "fwd.tile_h": 128}),
    Case("f4_whole_1440_137x141", 64, 512, [(137, 141)], True, "relu", True, "F(4x4), 128-row: whole-tile ranges (1440 tiles, 3 per workgroup within 16 %)",
         {"tile": 4, "fwd.n_tiles": 1440, "fwd.schedule": "whole_ranges", "fwd.tile_h": 128, "fwd.G": 512}),
    Case("f4_rows64_whole_1440_117x117", 64, 320, [(117, 117)], True, "relu", True, "F(4x4), 64-row: whole-tile ranges (1440 tiles)",
         {"tile": 4, "fwd.n_tiles": 1440, "fwd.schedule": "whole_ranges", "fwd.tile_h": 64, "fwd.m_tiles": 5}),
    Case("f4_rows64_whole_bwd_117x117", 320, 64, [(117, 117)], False, "none", True, "F(4x4), 64-row: whole-tile ranges in the data gradient",
         {"tile": 4, "bwd_data.n_tiles": 1440, "bwd_data.schedule": "whole_ranges", "bwd_data.tile_h": 64}),
    Case("f2_exactly_G", 64, 512, L8_SMALL, True, "relu", True, "F(2x2), 128-row: n_tiles = G = 512 exactly: one tile per workgroup; strips settle on per_block = 1024",
         {"tile": 2, "tg": 64, "fwd.n_tiles": 512, "fwd.G": 512, "fwd.schedule": "one_tile", "fwd.tile_h": 128, "strips_out.per_block": 1024}),
    Case("f2_three_quarters_G", 64, 384, L8_SMALL, True, "relu", True, "F(2x2), 128-row: n_tiles = 384 = 3/4 G exactly: one tile per workgroup",
         {"tile": 2, "fwd.n_tiles": 384, "fwd.G": 384, "fwd.schedule": "one_tile", "fwd.tile_h": 128}),
    Case("f2_rows64_three_quarters_G", 64, 192, L8_SMALL, True, "relu", True, "F(2x2), 64-row: n_tiles = 384 = 3/4 G exactly: one tile per workgroup",
         {"tile": 2, "fwd.n_tiles": 384, "fwd.schedule": "one_tile", "fwd.tile_h": 64}),
    Case("f2_streamk_256", 64, 256, L8_SMALL, False, "none", True, "F(2x2), 128-row: 256 tiles, below 3/4 G: stream-K",
         {"tile": 2, "fwd.n_tiles": 256, "fwd.schedule": "stream_k", "fwd.tile_h": 128, "fwd.G": 512}),
    Case("f2_rows64_band_640", 64, 320, L8_SMALL, True, "relu", True, "F(2x2), 64-row: 640 tiles in the G .. 2 G band: stream-K",
         {"tile": 2, "fwd.n_tiles": 640, "fwd.schedule": "stream_k", "fwd.tile_h": 64}),
    Case("f2_exactly_2G_whole", 64, 1024, L8_SMALL, True, "relu", True, "F(2x2), 128-row: n_tiles = 2 G exactly: whole-tile ranges, two tiles each",
         {"tile": 2, "fwd.n_tiles": 1024, "fwd.schedule": "whole_ranges", "fwd.tile_h": 128, "fwd.G": 512}),
    Case("f2_rows64_whole_1408", 64, 704, L8_SMALL, False, "relu", True, "F(2x2), 64-row: whole-tile ranges (1408 tiles, 3 per workgroup within 16 %)",
         {"tile": 2, "fwd.n_tiles": 1408, "fwd.schedule": "whole_ranges", "fwd.tile_h": 64}),
    Case("f2_exactly_G_bwd", 512, 64, L8_SMALL, True, "relu", True, "F(2x2): the data gradient at n_tiles = G exactly",
         {"tile": 2, "bwd_data.n_tiles": 512, "bwd_data.G": 512, "bwd_data.schedule": "one_tile", "bwd_data.tile_h": 128}),
]

# Plan classes the rules cannot reach at any shape (without FRCNN_WINO_M forcing a tile size), and why: the host test checks that the table covers every
# OTHER value, and that no case of the table or of the grid it walks lands in one of these.
UNREACHABLE = {
    "F(4x4) strips with per_block above 512": "Wn<4>::TPB = 512 is where its search starts",
    "weight gradient on whole-tile ranges or one tile per workgroup": "wn_wgrad_product always cuts its K range (the padded tile total) across workgroups: stream-K only",
    "fused 64 -> 64 product on F(2x2)": "rpn_wino_gemm_out64_kernel exists for the 4 x 4 tile only; a 64 -> 64 layer on F(2x2) runs the 64 x tg product",
    "pooled forms on F(2x2)": "the fused max-pool lives in the 4 x 4 tile's output transform: the entry points refuse relu = 2 / pooled = 1 on F(2x2)",
}


def get(plan, path):
    """plan["a"]["b"][0]["c"] for "a.b.0.c" """
    v = plan
    for k in path.split("."):
        v = v[int(k)] if isinstance(v, list) else v[k]
    return v
