"""The widths (K0, K1) and candidate counts N at which the 64 x 64 criterion tile (torchkge_amd/csrc/lp_tile64.h, behind
lp_xent.hip and lp_bce.hip) changes its column-slice, wave-tile, staging or chunk geometry -- test-only.

Every row names the bucket it is MEANT to hit; verify() holds each claim with plain integer arithmetic that mirrors the
kernels, and the chunk count against the library's own kge_lp_xent_chunks / kge_lp_bce_chunks (host arithmetic, no
device), so a changed constant in the headers or the wrappers moves the shapes or turns the table red instead of leaving
it silently stale.  tests/test_gpu_tile64_matrix.py calls verify() when it is collected, tests/test_tile64_table_host.py
without a GPU.

Everything is derived from the constants the headers publish (torchkge_amd._hip_xent / _hip_bce: BM, BN,
MIN_TILES_PER_CHUNK, MAX_CHUNKS, MAX_K, KSLICE).  Three numbers of lp_tile64.h are not published and are restated here:
the 32 columns of an MFMA tile (WT), the 4 waves of a block (WAVES) and the BK = 32 of a staging step, 8 k per MFMA block
(the widths below that are plain literals are positions relative to those).

The geometry, as the kernels have it:

  chunks(N)      min(MAX_CHUNKS, ceil(T / MIN_TILES_PER_CHUNK)), T = ceil(N / BN); chunk j = tiles [T j // chunks, T (j+1) // chunks)
  column slices  ceil((K0 + K1) / KSLICE) (blockIdx.z); slice z owns the columns [z KSLICE, (z+1) KSLICE) of segment 0 followed
                 by segment 1
  wave tiles     inside a slice wave w owns the 32-column tiles 4 ct + w, ct = 0 .. KSLICE/128 - 1, whose first column is
                 < K0 + K1; nct = the number of them; a lane's column switches to segment 1 at j >= K0
  staging        score_tile: BK = 32 columns of ONE segment per step, 8-blocks of 4 + 4 (k = 0,4,1,5,..), min(4, ceil(rest / 8))
                 blocks of the last step; 16-byte pieces (VEC4) when every segment's K is a multiple of 4 and the rows are
                 16-byte aligned, scalar loads otherwise
"""
WT, WAVES, BK = 32, 4, 32

# ---- K buckets -------------------------------------------------------------------------------------------------------
ONE_COL_SLICE1 = 'one column in slice 1: only wave 0 has work there, the other three waves have nct = 0'
SEG_BEFORE_SLICE = 'segment boundary one column before the slice boundary'
SEG_ON_SLICE = 'segment boundary exactly on the slice boundary, one column in slice 1'
SEG0_PAST_SLICE = 'K0 > KSLICE: slice 1 starts inside segment 0 and switches segment at an unaligned column'
SLICE_IN_SEG1 = 'slice boundary inside segment 1, at a column of it that is no multiple of 32'
WIDEST = 'the widest problem'
WIDEST_SEG_LATE = 'the widest problem, segment boundary one column before the end'
WIDEST_SEG_EARLY = 'the widest problem, segment boundary after one column'
NCT_GROWS_W0 = 'one column past whole wave tiles: nct grows by one for wave 0 only'
WHOLE_WAVE_TILES = 'whole 32-column wave tiles only'
VEC4_K4 = 'VEC4 with K % 8 == 4: the last 16-byte piece is half an 8-block'
WHOLE_STEPS = 'whole BK steps, nothing partial'
SCALAR_STEP_EDGE = 'scalar path one column around a BK step'
MIXED_VEC = 'one segment vectorisable, the other not: scalar path for both'
VEC4_K4_BOTH = 'VEC4 in both segments, K % 8 == 4 in both'
SEG1_AFTER_PARTIAL = 'segment 1 continues the accumulator after a partial step of segment 0'

SLICE, WAVE, STAGING = 'slice', 'wave', 'staging'      # what a row is in the table for (the GPU module's selections)


def k_table(x):
    """[(K0, K1, group, bucket)] from the published constants of `x` (torchkge_amd._hip_xent or _hip_bce)."""
    KS, MK = x.KSLICE, x.MAX_K
    return [
        (KS + 1, 0, SLICE, ONE_COL_SLICE1),
        (KS - 1, 1, SLICE, SEG_BEFORE_SLICE),
        (KS, 1, SLICE, SEG_ON_SLICE),
        (KS + 8, 8, SLICE, SEG0_PAST_SLICE),
        (300, 300, SLICE, SLICE_IN_SEG1),
        (MK, 0, SLICE, WIDEST),
        (MK - 1, 1, SLICE, WIDEST_SEG_LATE),
        (1, MK - 1, SLICE, WIDEST_SEG_EARLY),
        (129, 0, WAVE, NCT_GROWS_W0),
        (257, 0, WAVE, NCT_GROWS_W0),
        (385, 0, WAVE, NCT_GROWS_W0),
        (128, 0, WAVE, WHOLE_WAVE_TILES),
        (160, 0, WAVE, WHOLE_WAVE_TILES),
        (4, 0, STAGING, VEC4_K4),
        (12, 0, STAGING, VEC4_K4),
        (36, 0, STAGING, VEC4_K4),
        (100, 0, STAGING, VEC4_K4),
        (32, 0, STAGING, WHOLE_STEPS),
        (64, 0, STAGING, WHOLE_STEPS),
        (31, 0, STAGING, SCALAR_STEP_EDGE),
        (35, 0, STAGING, SCALAR_STEP_EDGE),
        (65, 0, STAGING, SCALAR_STEP_EDGE),
        (8, 5, STAGING, MIXED_VEC),
        (5, 8, STAGING, MIXED_VEC),
        (36, 12, STAGING, VEC4_K4_BOTH),
        (31, 33, STAGING, SEG1_AFTER_PARTIAL),
    ]


def four_slice_rows(x):
    """The rows that also run with three row panels and two chunks."""
    return [(x.KSLICE + 1, 0), (x.KSLICE + 8, 8), (300, 300), (x.MAX_K - 1, 1)]


def slices(x, K0, K1):
    return -(-(K0 + K1) // x.KSLICE)


def wave_tiles(x, K0, K1, z, w):
    """The 32-column tiles (numbered inside slice z) wave w owns -- grad_walk's `if (jt < Ktot) nct = ct + 1`."""
    CT = x.KSLICE // WT // WAVES
    return [WAVES * ct + w for ct in range(CT) if z * x.KSLICE + (WAVES * ct + w) * WT < K0 + K1]


def nct(x, K0, K1, z):
    return tuple(len(wave_tiles(x, K0, K1, z, w)) for w in range(WAVES))


def vec4(K0, K1):
    """operands_vec4() for dense 16-byte aligned segments (ld = K)."""
    return K0 % 4 == 0 and K1 % 4 == 0


def steps(K0, K1):
    """[(segment, k of the step's first column, 8-blocks the MFMA loop runs)] of score_tile, in order."""
    out = []
    for seg, K in ((0, K0), (1, K1)):
        for s in range(-(-K // BK)):
            out.append((seg, s * BK, min(4, (K - s * BK + 7) >> 3)))
    return out


# ---- N buckets -------------------------------------------------------------------------------------------------------
def chunks(x, N):
    """The header's formula."""
    return min(x.MAX_CHUNKS, -(-(-(-N // x.BN)) // x.MIN_TILES_PER_CHUNK))


def chunk_tiles(x, N):
    """[(first tile, one past the last tile)] of every chunk -- the `it0`, `it1` of grad_walk and the stats kernels."""
    T, c = -(-N // x.BN), chunks(x, N)
    return [(T * j // c, T * (j + 1) // c) for j in range(c)]


def chunk_cols(x, N):
    """The first candidate of every chunk, and N: [c_0 = 0, c_1, .., c_chunks = N]."""
    return [t0 * x.BN for t0, _ in chunk_tiles(x, N)] + [N]


def n_table(x):
    """[(N, T, chunks, chunk sizes in tiles, additive, bucket)].  `additive`: every chunk has at most MIN_TILES_PER_CHUNK
    tiles, so its candidate slice taken alone is ONE chunk and the full dA is the ascending sum of the slices' dA."""
    BN, M, C = x.BN, x.MIN_TILES_PER_CHUNK, x.MAX_CHUNKS
    return [
        ((3 * M - 3) * BN + 1, 3 * M - 2, 3, (M - 1, M - 1, M), True,
         'three unequal chunks, one long; last tile holds one candidate'),
        ((3 * M - 2) * BN + BN - 1, 3 * M - 1, 3, (M - 1, M, M), True,
         'three unequal chunks, one short; last tile lacks one candidate'),
        (M * (C - 1) * BN + BN // 2 + 5, M * (C - 1) + 1, C, None, True,
         'the first N with MAX_CHUNKS chunks: two chunk sizes below the cap; last tile partial'),
        (M * C * BN, M * C, C, (M,) * C, True,
         'full cap: all chunks equal, no partial tile'),
        (M * C * BN + 5, M * C + 1, C, None, False,
         'past the cap: exactly one chunk of MIN_TILES_PER_CHUNK + 1 tiles; last tile holds 5 candidates'),
        ((M * C + 4) * BN + BN - 1, M * C + 5, C, None, False,
         'past the cap: two chunk sizes mixed'),
    ]


def n_row(x, T):
    return next(r for r in n_table(x) if r[1] == T)


def verify(xent, bce):
    """Every claim of both tables against the constants and the library (torchkge_amd._hip_xent / _hip_bce; no GPU)."""
    names = ('BM', 'BN', 'MIN_TILES_PER_CHUNK', 'MAX_CHUNKS', 'MAX_K', 'KSLICE')
    assert [getattr(xent, n) for n in names] == [getattr(bce, n) for n in names], 'the two criteria publish one geometry'
    x = xent
    BM, BN, M, C, MK, KS = (getattr(x, n) for n in names)
    assert KS % (WT * WAVES) == 0 and KS < MK <= 2 * KS and M >= 3 and C >= 3
    assert BM + 1 >= C + 2      # the label rows of the N matrix: one per chunk boundary, the all-pairs row, the hub
    lib_x, lib_b = xent.load_library(), bce.load_library()

    # ---- K rows ----
    rows = k_table(x)
    assert len({(r[0], r[1]) for r in rows}) == len(rows)
    assert all(kk in {(r[0], r[1]) for r in rows if r[2] == SLICE} for kk in four_slice_rows(x))
    for K0, K1, group, why in rows:
        tag = 'K = %d + %d (%s)' % (K0, K1, why)
        Ktot = K0 + K1
        assert K0 >= 1 and K1 >= 0 and Ktot <= MK, tag
        ns = slices(x, K0, K1)
        assert ns == (Ktot + KS - 1) // KS and (ns == 2) == (Ktot > KS), tag
        assert (group == SLICE) == (Ktot >= KS), tag        # the slice rows: a full first slice, with or without a second
        # the wave tiles partition the columns: every column j < Ktot is lane l of exactly one (slice, wave, tile)
        owner = [0] * Ktot
        for z in range(ns):
            for w in range(WAVES):
                tiles = wave_tiles(x, K0, K1, z, w)
                assert tiles == [WAVES * ct + w for ct in range(len(tiles))], tag      # nct = a prefix of ct
                for t in tiles:
                    for l in range(WT):
                        j = z * KS + t * WT + l
                        if j < min(Ktot, (z + 1) * KS):
                            owner[j] += 1
        assert owner == [1] * Ktot, tag
        n0, n1 = nct(x, K0, K1, 0), (nct(x, K0, K1, 1) if ns == 2 else None)
        st = steps(K0, K1)
        assert sum(min(BK, (K0, K1)[seg] - k) for seg, k, _ in st) == Ktot, tag
        assert all(nb == -(-min(BK, (K0, K1)[seg] - k) // 8) for seg, k, nb in st), tag
        if why == ONE_COL_SLICE1:
            assert K1 == 0 and Ktot - KS == 1 and n1 == (1, 0, 0, 0), tag
        elif why == SEG_BEFORE_SLICE:
            assert K0 == KS - 1 and Ktot == KS and ns == 1, tag
        elif why == SEG_ON_SLICE:
            assert K0 == KS and K1 == 1 and n1 == (1, 0, 0, 0), tag
        elif why == SEG0_PAST_SLICE:
            assert K0 > KS and K1 > 0 and (K0 - KS) % WT != 0 and vec4(K0, K1), tag
            assert n1[0] == 1 and (K0 - KS) < WT and Ktot - KS < WT, tag       # the switch is inside wave 0's first tile
        elif why == SLICE_IN_SEG1:
            assert K0 < KS < Ktot and (KS - K0) % WT != 0 and K0 % WT != 0, tag
        elif why == WIDEST:
            assert (K0, K1) == (MK, 0) and n1 == (KS // WT // WAVES,) * WAVES, tag
        elif why == WIDEST_SEG_LATE:
            assert (K0, K1) == (MK - 1, 1), tag
        elif why == WIDEST_SEG_EARLY:
            assert (K0, K1) == (1, MK - 1), tag
        elif why == NCT_GROWS_W0:
            assert K1 == 0 and K0 % (WT * WAVES) == 1 and n0 == (n0[1] + 1, n0[1], n0[1], n0[1]) and n0[1] >= 1, tag
        elif why == WHOLE_WAVE_TILES:
            assert K1 == 0 and K0 % WT == 0, tag
        elif why == VEC4_K4:
            assert K1 == 0 and vec4(K0, K1) and K0 % 8 == 4, tag
        elif why == WHOLE_STEPS:
            assert K1 == 0 and K0 % BK == 0 and all(nb == 4 for _, _, nb in st), tag
        elif why == SCALAR_STEP_EDGE:
            assert K1 == 0 and not vec4(K0, K1) and 0 < min(K0 % BK, BK - K0 % BK) <= 3, tag
        elif why == MIXED_VEC:
            assert (K0 % 4 == 0) != (K1 % 4 == 0) and not vec4(K0, K1), tag
        elif why == VEC4_K4_BOTH:
            assert vec4(K0, K1) and K0 % 8 == 4 and K1 % 8 == 4, tag
        elif why == SEG1_AFTER_PARTIAL:
            assert K0 % BK != 0 and K1 > BK and K1 % BK != 0, tag
        else:
            raise AssertionError('no claim for ' + tag)
    widths = {(r[0], r[1]) for r in rows}
    assert {(129, 0), (257, 0), (385, 0)} <= widths and {(KS - 1, 1), (KS, 1)} <= widths
    assert len({nct(x, k, 0, 0) for k in (129, 257, 385)}) == 3         # wave 0 at three different tile counts

    # ---- N rows ----
    seen_T = set()
    for N, T, c, sizes, additive, why in n_table(x):
        tag = 'N = %d (%s)' % (N, why)
        assert N >= 1 and -(-N // BN) == T and T not in seen_T, tag
        seen_T.add(T)
        assert chunks(x, N) == c == int(lib_x.kge_lp_xent_chunks(N)) == int(lib_b.kge_lp_bce_chunks(N)), tag
        assert xent.chunks(N) == c and bce.chunks(N) == c, tag
        ct = chunk_tiles(x, N)
        assert ct[0][0] == 0 and ct[-1][1] == T and all(a[1] == b[0] for a, b in zip(ct, ct[1:])), tag
        got = tuple(t1 - t0 for t0, t1 in ct)
        assert min(got) >= 1, tag
        if sizes is not None:
            assert got == sizes, tag
        assert additive == (max(got) <= M), tag
        cols = chunk_cols(x, N)
        assert len(cols) == c + 1 and cols == sorted(set(cols)) and cols[-1] == N, tag
        if additive:    # a chunk's candidates alone: one chunk, walked from its tile 0
            for c0, c1 in zip(cols, cols[1:]):
                assert chunks(x, c1 - c0) == 1 == int(lib_b.kge_lp_bce_chunks(c1 - c0)), tag
    by_T = {r[1]: r for r in n_table(x)}
    assert len(by_T[3 * M - 2][3]) == 3 and len(set(by_T[3 * M - 2][3])) == 2 and len(set(by_T[3 * M - 1][3])) == 2
    for T in (3 * M - 2, 3 * M - 1, M * (C - 1) + 1, M * C + 1, M * C + 5):
        assert by_T[T][0] % BN != 0       # last tile partial
    assert by_T[M * C][0] % BN == 0 and by_T[M * C + 1][0] % BN == 5
    first_cap = by_T[M * (C - 1) + 1]
    assert chunks(x, (first_cap[1] - 1) * BN) == C - 1      # one tile fewer: one chunk fewer
    assert set(t1 - t0 for t0, t1 in chunk_tiles(x, first_cap[0])) == {M - 1, M}
    past1 = [t1 - t0 for t0, t1 in chunk_tiles(x, by_T[M * C + 1][0])]
    assert sorted(past1) == [M] * (C - 1) + [M + 1]
    past5 = [t1 - t0 for t0, t1 in chunk_tiles(x, by_T[M * C + 5][0])]
    assert set(past5) == {M, M + 1} and past5.count(M + 1) == 5
    # the library against the formula around every edge of the table, not only on its rows
    for N in sorted({n + d for n in [r[0] for r in n_table(x)] + [BN * M, BN * M * (C - 1)] for d in (-BN, -1, 0, 1, BN)}):
        if N >= 1:
            assert chunks(x, N) == int(lib_x.kge_lp_xent_chunks(N)) == int(lib_b.kge_lp_bce_chunks(N)), N
