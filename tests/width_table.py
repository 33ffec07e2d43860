"""The row widths K at which the count sweeps of the split prefilter change kernel, layout or launch shape -- test-only.

Every row of TABLE names the bucket its width is MEANT to hit; verify() holds each claim against the library's pure functions
(kge_lp_split_units, kge_lp_hi_units, kge_lp_hi_stream_supported, kge_lp_split_regions_supported) and (K + 17) // 16, so a
changed constant in torchkge_amd/csrc turns the table red instead of leaving it silently stale.  tests/test_gpu_width_matrix.py
calls verify() when it is collected, tests/test_width_table_host.py without a GPU.

The edges, as the dispatch has them today (kge_lp_split_count, lp_split_operands.hip, lp_hi_stream.hip, lp_hi_chunk.hip):

  three-product level   units = (K + 16) // 16 (K columns + 1 augmentation column), units_p = units rounded up to 2
  one-product level     units = (K + 17) // 16 (K columns + 2 augmentation columns), units_p = units rounded up to 4
  free-running kernel   units <= 32 (resident query panel); bodies specialised for 13 and 26 units, a runtime loop otherwise
  chunked-panel kernel  exactly 33 and 65 units, plain thresholds only
  planar kernel         everything else (34..64, 66 and up) and every projection-mode problem past 32 units
  augmentation columns  one-product level: K % 16 <= 13 they SHARE the last data unit, == 14 they FILL it, == 15 they STRADDLE
                        into the next unit, == 0 both open the NEXT unit;  three-product level (one column): <= 14 share,
                        == 15 fill, == 0 next
  builder tiles         16 rows x 16 cells: one more tile column whenever units_p crosses a multiple of 16
  prefix maxima         kge_lp_split_prefix_max refuses units_p > 128, i.e. K >= 2048 ((2047 + 16) // 16 = 128 still fits;
                        the "(K <= 2031)" beside that check counts the unit the augmentation column does not need)

4-wave / 8-wave flip of kge_hi_stream_launch: two 4-wave workgroups per CU while 2 * smem4 <= 160 KiB - 2 KiB, with
  smem4 = tq * (32 * units + 16) + 4 * 384 * 8 + tq * sets * 20      (panel + four waves' lists + thresholds and rows)
  plain thresholds  (tq = 128, sets = 1): 4096 u + 16896 <= 80896  <=>  u <= 15   -> 15 | 16 units, K = 238 | 239
  projection modes  (tq =  96, sets = 1): 3072 u + 15744 <= 80896  <=>  u <= 21   -> 21 | 22 units, K = 334 | 335
  grouped columns   (tq =  96, sets = 4): 3072 u + 21504 <= 80896  <=>  u <= 19   -> 19 | 20 units, K = 302 | 303
"""
import ctypes

# one-product routes of the PLAIN-threshold forms (KGE_LP_L2_EXPAND / KGE_LP_DOT) on a fragment-major table
S13, S26, LOOP, CHUNK, PLANAR = 'stream<13>', 'stream<26>', 'stream<loop>', 'chunked', 'planar-only'
SHARE, FILL, STRADDLE, NEXT = 'share', 'fill', 'straddle', 'next'

# (K, three-product units_p, one-product units, one-product units_p, route, augmentation columns on the one-product level,
#  waves per workgroup of the free-running kernel (plain, projection) or None, what the width is in the table for)
TABLE = [
    (1,    2,   1,   4,   LOOP,   SHARE,    (4, 4), 'the smallest row'),
    (13,   2,   1,   4,   LOOP,   SHARE,    (4, 4), 'augmentation pair in the last two free columns but one'),
    (14,   2,   1,   4,   LOOP,   FILL,     (4, 4), 'augmentation pair fills the data unit exactly'),
    (15,   2,   2,   4,   LOOP,   STRADDLE, (4, 4), 'augmentation pair straddles units 0 | 1; three products: fills'),
    (16,   2,   2,   4,   LOOP,   NEXT,     (4, 4), 'augmentation columns open their own unit'),
    (17,   2,   2,   4,   LOOP,   SHARE,    (4, 4), 'one data column in the second unit'),
    (24,   2,   2,   4,   LOOP,   SHARE,    (4, 4), 'model level: the smallest d % 8 == 0 past one unit'),
    (64,   6,   5,   8,   LOOP,   NEXT,     (4, 4), 'model level: the width the other tests use'),
    (184,  12,  12,  12,  LOOP,   SHARE,    (4, 4), 'model level: below the 13-unit body'),
    (190,  12,  12,  12,  LOOP,   FILL,     (4, 4), 'last width below the 13-unit body'),
    (191,  12,  13,  16,  S13,    STRADDLE, (4, 4), 'first width of the 13-unit body'),
    (192,  14,  13,  16,  S13,    NEXT,     (4, 4), 'model level: first admissible width of the 13-unit body'),
    (200,  14,  13,  16,  S13,    SHARE,    (4, 4), 'model level: the flagship width'),
    (203,  14,  13,  16,  S13,    SHARE,    (4, 4), 'model level: d % 8 != 0, the general path'),
    (205,  14,  13,  16,  S13,    SHARE,    (4, 4), 'straddle series inside the 13-unit body'),
    (206,  14,  13,  16,  S13,    FILL,     (4, 4), 'last width of the 13-unit body'),
    (207,  14,  14,  16,  LOOP,   STRADDLE, (4, 4), '14 units must NOT take the 13-unit body'),
    (208,  14,  14,  16,  LOOP,   NEXT,     (4, 4), 'model level: first admissible width past the 13-unit body'),
    (232,  16,  15,  16,  LOOP,   SHARE,    (4, 4), 'model level: 4-wave side of the plain flip'),
    (238,  16,  15,  16,  LOOP,   FILL,     (4, 4), 'plain thresholds: last width on two 4-wave workgroups'),
    (239,  16,  16,  16,  LOOP,   STRADDLE, (8, 4), 'plain thresholds: first width on one 8-wave workgroup'),
    (240,  16,  16,  16,  LOOP,   NEXT,     (8, 4), 'model level: 8-wave side of the plain flip'),
    (254,  16,  16,  16,  LOOP,   FILL,     (8, 4), 'one-product units_p = 16: last width of one builder tile column'),
    (255,  16,  17,  20,  LOOP,   STRADDLE, (8, 4), 'one-product units_p crosses 16; three products: last of units_p = 16'),
    (256,  18,  17,  20,  LOOP,   NEXT,     (8, 4), 'three-product units_p crosses 16'),
    (302,  20,  19,  20,  LOOP,   FILL,     (8, 4), 'grouped columns: last width on 4-wave workgroups'),
    (303,  20,  20,  20,  LOOP,   STRADDLE, (8, 4), 'grouped columns: first width on an 8-wave workgroup'),
    (328,  22,  21,  24,  LOOP,   SHARE,    (8, 4), 'model level: 4-wave side of the projection flip'),
    (332,  22,  21,  24,  LOOP,   SHARE,    (8, 4), 'projection modes (K % 4 == 0): last width on 4-wave workgroups'),
    (334,  22,  21,  24,  LOOP,   FILL,     (8, 4), 'last width of 21 units'),
    (335,  22,  22,  24,  LOOP,   STRADDLE, (8, 8), 'first width of 22 units'),
    (336,  22,  22,  24,  LOOP,   NEXT,     (8, 8), 'projection modes: first width on an 8-wave workgroup'),
    (392,  26,  25,  28,  LOOP,   SHARE,    (8, 8), 'model level: below the 26-unit body'),
    (398,  26,  25,  28,  LOOP,   FILL,     (8, 8), 'last width below the 26-unit body'),
    (399,  26,  26,  28,  S26,    STRADDLE, (8, 8), 'first width of the 26-unit body'),
    (400,  26,  26,  28,  S26,    NEXT,     (8, 8), 'model level: first admissible width of the 26-unit body'),
    (408,  26,  26,  28,  S26,    SHARE,    (8, 8), 'model level: last admissible width of the 26-unit body'),
    (414,  26,  26,  28,  S26,    FILL,     (8, 8), 'last width of the 26-unit body'),
    (415,  26,  27,  28,  LOOP,   STRADDLE, (8, 8), '27 units must NOT take the 26-unit body'),
    (416,  28,  27,  28,  LOOP,   NEXT,     (8, 8), 'model level: first admissible width past the 26-unit body'),
    (495,  32,  32,  32,  LOOP,   STRADDLE, (8, 8), 'first width of 32 units: the longest resident panel'),
    (496,  32,  32,  32,  LOOP,   NEXT,     (8, 8), 'model level: first admissible width of 32 units'),
    (504,  32,  32,  32,  LOOP,   SHARE,    (8, 8), 'model level: last admissible resident panel'),
    (510,  32,  32,  32,  LOOP,   FILL,     (8, 8), 'last width of the resident panel'),
    (511,  32,  33,  36,  CHUNK,  STRADDLE, None,   'first width of the 33-unit chunked panel; one-product units_p crosses 32'),
    (512,  34,  33,  36,  CHUNK,  NEXT,     None,   'three-product units_p crosses 32; model level: TransH / TransD keep planar'),
    (520,  34,  33,  36,  CHUNK,  SHARE,    None,   'model level: last admissible 33-unit width'),
    (526,  34,  33,  36,  CHUNK,  FILL,     None,   'last width of the 33-unit chunked panel'),
    (527,  34,  34,  36,  PLANAR, STRADDLE, None,   '34 units: planar only'),
    (528,  34,  34,  36,  PLANAR, NEXT,     None,   'model level: first admissible planar-only width'),
    (600,  38,  38,  40,  PLANAR, SHARE,    None,   'mid range: planar only'),
    (1016, 64,  64,  64,  PLANAR, SHARE,    None,   'model level: 64 units'),
    (1022, 64,  64,  64,  PLANAR, FILL,     None,   'last width of 64 units'),
    (1023, 64,  65,  68,  CHUNK,  STRADDLE, None,   'first width of the 65-unit chunked panel'),
    (1024, 66,  65,  68,  CHUNK,  NEXT,     None,   'model level: TransH / TransD keep planar'),
    (1032, 66,  65,  68,  CHUNK,  SHARE,    None,   'model level: last admissible 65-unit width'),
    (1038, 66,  65,  68,  CHUNK,  FILL,     None,   'last width of the 65-unit chunked panel'),
    (1039, 66,  66,  68,  PLANAR, STRADDLE, None,   '66 units: planar only'),
    (1040, 66,  66,  68,  PLANAR, NEXT,     None,   'model level: planar only'),
    (2028, 128, 127, 128, PLANAR, SHARE,    None,   'both units_p = 128: the widest prefix-maxima operand'),
    (2032, 128, 128, 128, PLANAR, NEXT,     None,   'ComplEx d = 1016: three-product units_p still 128'),
    (2047, 128, 129, 132, PLANAR, STRADDLE, None,   'last width kge_lp_split_prefix_max takes'),
    (2048, 130, 129, 132, PLANAR, NEXT,     None,   'ComplEx d = 1024: three products without prefix maxima'),
]

ROW = {row[0]: row for row in TABLE}
WIDTHS = [row[0] for row in TABLE]
PANEL_UNITS = 32            # the resident panel (= torchkge_amd._hip.HI_STREAM_PANEL_UNITS; verify() holds both to the library)
PREFIX_MAX_UNITS = 128      # (= torchkge_amd._hip.SPLIT_PREFIX_MAX_UNITS)


def units1(K):
    return (K + 17) // 16


def route(K):
    return ROW[K][4]


def frag_ok(K, proj=False):
    """Does the table send this width to a fragment-major sweep (plain thresholds / a projection mode)?"""
    r = route(K)
    return r in (S13, S26, LOOP) or (r == CHUNK and not proj)


def waves(units, tq, sets):
    """Workgroup size kge_hi_stream_launch picks -- the LDS expression of the module docstring."""
    smem4 = (tq * (32 * units + 16) + 15) // 16 * 16 + 4 * 384 * 8 + tq * sets * 20
    return 4 if 2 * smem4 <= 160 * 1024 - 2048 else 8


def aug1(K):
    r = K % 16
    return NEXT if r == 0 else (SHARE if r <= 13 else (FILL if r == 14 else STRADDLE))


def verify(hip):
    """Every claim of TABLE against the library (`hip` = torchkge_amd._hip, loaded; no GPU needed)."""
    lib = hip.load_library()
    assert hip.HI_STREAM_PANEL_UNITS == PANEL_UNITS and hip.SPLIT_PREFIX_MAX_UNITS == PREFIX_MAX_UNITS
    assert sorted(set(WIDTHS)) == WIDTHS
    for K, u0p, u1, u1p, rt, aug, wv, why in TABLE:
        tag = 'K = %d (%s)' % (K, why)
        assert int(lib.kge_lp_split_units(K, 1)) == u0p, tag
        assert units1(K) == u1, tag
        assert int(lib.kge_lp_hi_units(K)) == u1p and u1p % 4 == 0 and 0 <= u1p - u1 < 4, tag
        assert aug1(K) == aug, tag
        # the pair's second column sits in the unit after K's exactly when it straddles or opens the next unit
        assert ((K + 1) // 16 > (K - 1) // 16) == (aug in (STRADDLE, NEXT)), tag
        assert int(lib.kge_lp_hi_stream_supported(K)) == (1 if rt != PLANAR else 0), tag
        assert bool(hip.hi_stream_ok(K)) == (rt != PLANAR) or not hip.HI_STREAM, tag
        assert hip.hi_stream_panel_ok(K) == (rt in (S13, S26, LOOP)) == (u1 <= PANEL_UNITS), tag
        assert (rt == S13) == (u1 == 13) and (rt == S26) == (u1 == 26), tag
        assert (rt == CHUNK) == (u1 in (33, 65)), tag
        # kge_lp_split_regions_supported: the resident panel's range again, for float4-readable rows (a descriptor of
        # never-dereferenced, 16-byte aligned addresses: the function only looks at shapes and alignment)
        d = hip.LpDesc()
        d.mode, d.K0, d.K1, d.B, d.N = hip.LP_DOT, K, 0, 1, 1
        d.A0, d.T0, d.lda0, d.ldt0 = 4096, 8192, K, K
        assert int(lib.kge_lp_split_regions_supported(ctypes.byref(d))) == (1 if (K % 4 == 0 and u1 <= PANEL_UNITS) else 0), tag
        assert (wv is None) == (u1 > PANEL_UNITS), tag
        if wv is not None:
            assert wv == (waves(u1, 128, 1), waves(u1, 96, 1)), tag
        assert (u0p > PREFIX_MAX_UNITS) == (K >= 2048), tag
    # both sides of every edge are in the table
    for lo in (190, 206, 398, 414, 238, 334, 302, 254, 255, 510, 511, 526, 1022, 1038, 2047):
        assert lo in ROW and lo + 1 in ROW, lo
    assert waves(19, 96, 4) == 4 and waves(20, 96, 4) == 8
