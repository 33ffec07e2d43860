"""GPU tests of the three top-k selection kernels of torchkge_amd/csrc/topk.hip (run with -m gpu on an MI355X):
topk_chunk_reg_kernel<8 | 16 | 32> (the one-pass register selection behind kge_topk_chunk for k <= 32), topk_chunk_kernel
(its k-pass fallback: k > 32, or KGE_TOPK_REG=0) and topk_kernel (kge_topk).

What the cases are chosen for.  The one-pass kernel rebuilds its wave-wide pruning threshold at iterations 16, 64 and 256 of
the column loop, but only inside the unrolled part (steps of 8 x 64 columns), so the three refreshes first happen at
C = 1536, 4608 and 16896: every C list here holds both sides of those, of the unroll step (512) and of one iteration (64).
k = 1, 8 | 9, 16 | 17, 32 | 33 are the edges of the three register-list sizes and of the fallback.  The row families put
ties, constant rows, -inf, NaN, late winners and one-lane winners across those refreshes; the grid-cap cases have more rows
than 4096 blocks serve in one sweep (16384 rows for the one-pass kernel, 4096 for the other two).  Two families were
added to the eleven the cases started from, each for a wrong threshold the others let through: -inf entries that arrive
after a refresh at which fewer than k columns were selectable (a threshold of -inf switched on there would drop them), and
a k-th best that arrives last, between the (k-1)-th and the k-th score of every refresh (a threshold one rank too high
would drop it).

Reference: numpy on the host, vectorised over rows.  A column is selectable if its score is not NaN and, in merge mode,
its id is >= 0; the selectable columns are ordered by (score descending in float64, column ascending); the first k are
returned, slots past the number of selectable columns are (-inf, -1); -inf is selectable and comes out with its real id.
Every comparison is exact: ids as integers, values as int32 bit patterns, the tile after a call bit for bit (unchanged, or
with exactly the in-chunk targets set to -inf).  There is no tolerance anywhere in this module."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, raw, carve, guarded_out, assert_guard_intact

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
KGE_EINVAL = -1
FAMILIES = ['normal', 'quantised', 'constant', 'ascending', 'descending', 'late-winners', 'late-winners-behind-neginf',
            'all-neginf', 'all-nan', 'one-lane', 'specials', 'late-neginf-behind-nan',
            'kth-best-last']
ONE_PASS_C = [1, 63, 64, 65, 511, 512, 513, 1535, 1536, 1537, 4607, 4608, 4609, 16895, 16896, 16897]
ONE_PASS_K = [1, 8, 9, 16, 17, 32]
FALLBACK_C = [65, 1537, 16897]
SWITCH_CASES = [(C, k) for C in (513, 1537, 4609) for k in (8, 32)]
COL_OFF = 3


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------
# row families and the reference
# ---------------------------------------------------------------------------
def quantised(rng, C):
    return (rng.integers(-4, 4, C) / 8.0).astype(np.float32)        # eight levels: about C / 8 ties at each


def family_row(name, C, k, rng):
    """One fp32 row of width C of the family `name`, shaped for (C, k): "the last 40 columns" are the last min(40, C)."""
    tail = min(40, C)
    if name == 'normal':
        return rng.standard_normal(C).astype(np.float32)
    if name == 'quantised':
        return quantised(rng, C)
    if name == 'constant':
        return np.full(C, 0.375, np.float32)
    if name == 'ascending':                                         # (exact in fp32 up to C = 2^22)
        return (np.arange(C) * 0.25 - 7.0).astype(np.float32)
    if name == 'descending':
        return (7.0 - np.arange(C) * 0.25).astype(np.float32)
    if name == 'late-winners':      # fewer than k selectable columns at every refresh, the winners in the last iteration
        row = np.full(C, NAN, np.float32)
        row[C - tail:] = rng.standard_normal(tail).astype(np.float32)
        head = np.array([1.0, -INF, 2.0], np.float32)[:min(3, C)]
        row[:head.shape[0]] = head
        return row
    if name == 'late-winners-behind-neginf':    # a k-th entry of -inf at every refresh, small integers with ties at the end
        row = np.full(C, -INF, np.float32)
        row[C - tail:] = rng.integers(0, 5, tail).astype(np.float32)
        return row
    if name == 'all-neginf':
        return np.full(C, -INF, np.float32)
    if name == 'all-nan':
        return np.full(C, NAN, np.float32)
    if name == 'one-lane':          # the k largest values all in lane 5's columns, in no particular order
        row = rng.standard_normal(C).astype(np.float32)
        cols = 5 + 64 * np.arange(k)
        cols = cols[cols < C]
        row[cols] = (10.0 + rng.permutation(cols.shape[0])).astype(np.float32)
        return row
    if name == 'specials':
        row = quantised(rng, C)
        u = rng.random(C)
        row[u < 0.05] = INF
        row[(u >= 0.05) & (u < 0.10)] = NAN
        row[(u >= 0.10) & (u < 0.12)] = -INF
        return row
    if name == 'late-neginf-behind-nan':    # fewer than k selectable columns at every refresh AND -inf entries behind it:
        row = np.full(C, NAN, np.float32)   # they are selectable, whatever the threshold of an exhausted selection is
        row[C - tail:] = -INF
        row[[C - 1, C - 1 - 16 % tail, C - 1 - 29 % tail]] = rng.standard_normal(3).astype(np.float32)
        return row
    if name == 'kth-best-last':     # descending, but the k-th best sits in the last column: at every refresh it lies between
        row = (7.0 - np.arange(C) * 0.25).astype(np.float32)        # the (k-1)-th and the k-th score seen so far
        if k - 1 < C - 1:
            row[[k - 1, C - 1]] = row[[C - 1, k - 1]]
        return row
    raise KeyError(name)


def family_matrix(C, k, names=FAMILIES):
    rng = np.random.default_rng(1000003 * C + 101 * k)
    return np.stack([family_row(n, C, k, rng) for n in names])


def reference(S, k, ids=None, c_base=0):
    """(values (B, k) fp32, ids (B, k) int64) of the order (score descending in float64, column ascending) over the
    selectable columns; (-inf, -1) past their number.  Vectorised over rows."""
    B, C = S.shape
    s64 = S.astype(np.float64)
    sel = ~np.isnan(s64)
    if ids is not None:
        sel &= ids >= 0
    cols = np.broadcast_to(np.arange(C), (B, C))
    neg = np.where(sel, -s64, 0.0)
    order = np.lexsort((cols, neg, ~sel), axis=1)[:, :k]            # unselectable last, then score, then column
    if k > C:
        order = np.concatenate([order, np.zeros((B, k - C), order.dtype)], axis=1)
    valid = np.arange(k)[None, :] < sel.sum(1)[:, None]
    val = np.where(valid, np.take_along_axis(S, order, 1), np.float32(-INF)).astype(np.float32)
    out = np.take_along_axis(ids, order, 1) if ids is not None else order.astype(np.int64) + c_base
    return val, np.where(valid, out, -1).astype(np.int64)


def test_the_reference_orders_ties_neginf_and_nan_as_stated():
    S = np.array([[1.0, NAN, 1.0, -INF, 2.0], [NAN, NAN, -INF, NAN, NAN]], np.float32)
    val, idx = reference(S, 6, c_base=10)
    assert idx.tolist() == [[14, 10, 12, 13, -1, -1], [12, -1, -1, -1, -1, -1]]
    assert val.tolist() == [[2.0, 1.0, 1.0, -INF, -INF, -INF], [-INF] * 6]
    ids = np.array([[7, 9, -1, 11, -1], [-1] * 5], np.int64)
    val, idx = reference(S, 2, ids=ids)
    assert idx.tolist() == [[7, 11], [-1, -1]] and val.tolist() == [[1.0, -INF], [-INF, -INF]]


def first_bad_row(got_val, got_idx, ref_val, ref_idx):
    bad = (got_idx != ref_idx).any(1) | (bits(got_val) != bits(ref_val)).any(1)
    return int(np.argmax(bad)) if bad.any() else None


# ---------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------
def run_chunk(hip, S, k, c_base=0, seg=None, ids=None, expect_tile=None):
    """kge_topk_chunk on a (B, C) host matrix laid out as the tiled inference lays it out: the tile is the first C
    columns of a wider matrix (ld = C + 5, +inf in the pad and around it), the k best land in columns
    [COL_OFF, COL_OFF + k) of (B, COL_OFF + k + 2) outputs pre-filled with sentinels, ids_in has ld_ids = C + 3 with a
    real-looking id as poison.  seg = (seg_lo, seg_hi, targets).  Checks the guards and the tile; returns (values, ids)."""
    B, C = S.shape
    tile = carve(torch.from_numpy(S), 5, 0, INF, device='cuda')
    out_idx = guarded_out(B, COL_OFF + k, 2, 0, dtype=torch.int64)
    out_val = guarded_out(B, COL_OFF + k, 2, 0)
    assert tile.stride(0) > C and out_val.stride(0) > COL_OFF + k
    # (around the segments: empty ones, and a target that would mask column 0 wherever c_base fits an int32)
    d_seg = [None] * 3 if seg is None else [carve(torch.from_numpy(x), off=0, poison=p, device='cuda')
                                            for x, p in zip(seg, (0, 0, c_base if c_base < 2 ** 31 else 0))]
    d_ids = None if ids is None else carve(torch.from_numpy(ids), 3, 0, poison=10 ** 9, device='cuda')
    hip.topk_chunk(tile, c_base, k, out_val, out_idx, COL_OFF, d_seg[0], d_seg[1], d_seg[2], d_ids)
    torch.cuda.synchronize()
    assert_guard_intact(out_idx, col0=COL_OFF)
    assert_guard_intact(out_val, col0=COL_OFF)
    for v in [tile, d_ids] + d_seg:
        if v is not None:
            assert_guard_intact(v)
    if d_ids is not None:
        assert np.array_equal(d_ids.cpu().numpy(), ids)
    want = S if expect_tile is None else expect_tile
    assert np.array_equal(bits(tile.cpu().numpy()), bits(want)), 'the tile after the call'
    return out_val[:, COL_OFF:].cpu().numpy(), out_idx[:, COL_OFF:].cpu().numpy()


LAUNCHES = {}


def family_launch(hip, entry, C, k):
    """The one launch of `entry` on the family rows at (C, k), its reference and the reference's own sanity,
    shared by the tests of the families."""
    key = (entry, C, k)
    if key not in LAUNCHES:
        S = family_matrix(C, k)
        if entry == 'chunk':
            c_base = 1000
            val, idx = run_chunk(hip, S, k, c_base)
        else:
            c_base = 0
            v, i = hip.topk(torch.from_numpy(S).cuda(), k)
            val, idx = v.cpu().numpy(), i.cpu().numpy()
        LAUNCHES[key] = (val, idx) + reference(S, k, c_base=c_base)
    return LAUNCHES[key]


def check_family(hip, entry, C, k, family):
    val, idx, ref_val, ref_idx = family_launch(hip, entry, C, k)
    r = FAMILIES.index(family)
    assert idx.shape == (len(FAMILIES), k) and val.dtype == np.float32
    assert idx[r].tolist() == ref_idx[r].tolist(), (entry, C, k, family)
    assert bits(val[r]).tolist() == bits(ref_val[r]).tolist(), (entry, C, k, family)


def family_params(Cs, ks):
    return [pytest.param(C, k, f, id='C%d-k%d-%s' % (C, k, f)) for C in Cs for k in ks for f in FAMILIES]


# ---------------------------------------------------------------------------
# 1. the one-pass kernel over its column thresholds, the fallback kernel and kge_topk
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('C,k,family', family_params(ONE_PASS_C, ONE_PASS_K))
def test_one_pass_kernel_every_refresh_threshold_and_k_bucket(hip, C, k, family):
    """Both sides of one iteration (64 columns), one unrolled step (512) and the three refreshes of the pruning threshold
    (1536, 4608, 16896), k on both sides of every register-list size; k > C is legal and fills with (-inf, -1)."""
    check_family(hip, 'chunk', C, k, family)


@pytest.mark.parametrize('C,k,family', family_params(FALLBACK_C, [33, 40]))
def test_fallback_kernel_above_32(hip, C, k, family):
    check_family(hip, 'chunk', C, k, family)


@pytest.mark.parametrize('C,k,family', family_params(FALLBACK_C, [1, 9, 33]))
def test_kge_topk_on_the_same_rows(hip, C, k, family):
    check_family(hip, 'topk', C, k, family)


# ---------------------------------------------------------------------------
# 2. filter masking in place, global ids next to the int32 limit
# ---------------------------------------------------------------------------
def filter_case(C, k):
    """(S (7, C), seg_lo, seg_hi, targets int32, masked S) with c_base = 2^31 - 1 - C: the chunk's last global id is
    2^31 - 2, and 2^31 - 1 -- the largest int32 -- is the first id behind it."""
    rng = np.random.default_rng(77 * C + k)
    c_base = 2 ** 31 - 1 - C
    S = family_matrix(C, k, ['normal', 'quantised', 'specials', 'normal', 'quantised', 'one-lane', 'normal'])
    top = reference(S[6:7], k)[1][0]
    segs = [
        [],                                                                         # empty, at offset 0
        [c_base - 1, c_base - 5, 0, -3, c_base + 2, c_base + C // 2],               # below c_base (and negative), two inside
        [c_base + C - 1, c_base + C, c_base + 11, c_base + 11, c_base + 11],        # the last column, the first id behind, duplicates
        (c_base + rng.choice(C, 65, replace=False)).tolist(),                       # more than one target per lane
        (c_base + rng.permutation(C)[:300]).tolist(),                               # 300 targets: every column at C = 300
        [] if C == 300 else (c_base + rng.permutation(C)).tolist(),                 # every column (empty in the middle at C = 300)
        (c_base + top[top >= 0]).tolist(),                                          # exactly the unfiltered top k
    ]
    junk = [c_base + 1, c_base + 3]                     # in-chunk targets that belong to no row's segment
    targets, lo, hi = list(junk), [], []
    for s in segs:
        lo.append(len(targets))
        targets += s
        hi.append(len(targets))
        targets += junk
    targets = np.array(targets, np.int64)
    assert targets.max() == 2 ** 31 - 1 and targets.min() < 0
    masked = S.copy()
    for i, s in enumerate(segs):
        t = np.array(s, np.int64) - c_base
        masked[i, t[(t >= 0) & (t < C)]] = -INF
    every = 4 if C == 300 else 5
    assert bool(np.isneginf(masked[every]).all()) and not np.isneginf(masked[0]).any()
    return S, np.array(lo, np.int64), np.array(hi, np.int64), targets.astype(np.int32), masked, c_base, every


@pytest.mark.parametrize('k', [8, 32])
@pytest.mark.parametrize('C', [300, 1537, 4609])
def test_filter_masking_in_place_next_to_the_int32_limit(hip, C, k):
    """B = 7 (the last block has an inactive wave that must still reach the barrier; B = 5: three of them).  The tile after
    the call is the input with exactly the in-chunk targets at -inf (checked in run_chunk, NaNs bit for bit)."""
    S, lo, hi, targets, masked, c_base, every = filter_case(C, k)
    for B in (7, 5):
        ref_val, ref_idx = reference(masked[:B], k, c_base=c_base)
        val, idx = run_chunk(hip, S[:B], k, c_base, seg=(lo[:B], hi[:B], targets), expect_tile=masked[:B])
        bad = first_bad_row(val, idx, ref_val, ref_idx)
        assert bad is None, (C, k, 'B', B, 'row', bad, idx[bad].tolist(), ref_idx[bad].tolist())
        if every < B:       # the row whose segment masks every column: the first k ids, all at -inf
            assert idx[every].tolist() == (c_base + np.arange(k)).tolist() and bool(np.isneginf(val[every]).all())


@pytest.mark.parametrize('k', [8, 33])
@pytest.mark.parametrize('c_base', [2 ** 31 - 5, 2 ** 32 + 100], ids=['across-2p31', 'past-2p32'])
def test_global_ids_past_the_int32_limit(hip, c_base, k):
    """column + c_base is a 64-bit sum (ids across and past 2^31), and target - c_base a 64-bit difference: int32
    targets that equal the chunk's ids modulo 2^32 lie outside it and mask nothing."""
    C = 300
    S = family_matrix(C, k, ['normal', 'quantised', 'ascending', 'specials', 'all-neginf'])
    B = S.shape[0]
    wrapped = ((c_base + np.arange(6, C, 3)) % 2 ** 32).astype(np.int64)       # (ids >= 2^31: none is an int32 itself)
    wrapped = np.where(wrapped >= 2 ** 31, wrapped - 2 ** 32, wrapped).astype(np.int32)
    n = wrapped.shape[0]
    seg = (np.zeros(B, np.int64), np.full(B, n, np.int64), wrapped)
    ref_val, ref_idx = reference(S, k, c_base=c_base)
    assert int(ref_idx.max()) >= 2 ** 31
    val, idx = run_chunk(hip, S, k, c_base, seg=seg, expect_tile=S)
    bad = first_bad_row(val, idx, ref_val, ref_idx)
    assert bad is None, (c_base, k, 'row', bad, idx[bad].tolist(), ref_idx[bad].tolist())


# ---------------------------------------------------------------------------
# 3. merge mode
# ---------------------------------------------------------------------------
def merge_case(C, k):
    rng = np.random.default_rng(31 * C + k)
    S = family_matrix(C, k, ['quantised', 'normal', 'specials', 'quantised', 'normal', 'constant'])
    B = S.shape[0]
    step = (2 ** 41) // C
    ids = (np.arange(C, dtype=np.int64) * step)[None, :] + rng.integers(0, step, (B, C))    # ascending, gaps, past 2^40
    assert bool((np.diff(ids, axis=1) > 0).all()) and int(ids.max()) > 2 ** 40
    pad = rng.random((B, C)) < 0.3
    pad[3] = True                       # row 3: real ids only in the last 20 columns and column 7
    pad[3, C - 20:] = False
    pad[3, 7] = False
    pad[4] = True                       # row 4: no real id at all
    ids[pad] = -1
    under = rng.integers(0, 3, (B, C))  # under the padding ids: +inf, NaN and ordinary scores, none may be selected
    S[pad & (under == 0)] = INF
    S[pad & (under == 1)] = NAN
    return S, ids


@pytest.mark.parametrize('k', [8, 16, 32])
@pytest.mark.parametrize('C', [96, 1600, 4700])
def test_merge_mode_long_partial_lists_padding_ids_and_int64_ids(hip, C, k):
    S, ids = merge_case(C, k)
    ref_val, ref_idx = reference(S, k, ids=ids)
    assert bool((ref_idx[4] == -1).all()) and int((ref_idx[3] >= 0).sum()) == min(k, 21)
    val, idx = run_chunk(hip, S, k, 0, ids=ids)
    bad = first_bad_row(val, idx, ref_val, ref_idx)
    assert bad is None, (C, k, 'row', bad, idx[bad].tolist(), ref_idx[bad].tolist())


# ---------------------------------------------------------------------------
# 4. two levels end to end: per-tile lists, then the merge call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('k', [9, 32, 40])
@pytest.mark.parametrize('C', [7, 256, 1536, 'N'])
@pytest.mark.parametrize('N', [1203, 5000])
def test_tiled_selection_then_merge_equals_the_whole_row(hip, N, C, k):
    """(5, N) rows of the families with ties, late winners, -inf and NaN, cut into tiles of C columns (some smaller than
    k: their lists end in (-inf, -1) padding): the merged top k is the reference top k of the whole row."""
    C = N if C == 'N' else C
    S = family_matrix(N, k, ['quantised', 'late-winners', 'late-winners-behind-neginf', 'one-lane', 'specials'])
    ref_val, ref_idx = reference(S, k)
    d_S = torch.from_numpy(S).cuda()
    n_tiles = (N + C - 1) // C
    part_val = torch.full((5, n_tiles * k), NAN, device='cuda')
    part_idx = torch.full((5, n_tiles * k), 10 ** 9, dtype=torch.int64, device='cuda')
    for j in range(n_tiles):
        hip.topk_chunk(d_S[:, j * C:min(N, (j + 1) * C)], j * C, k, part_val, part_idx, j * k)
    val = torch.full((5, k), NAN, device='cuda')
    idx = torch.full((5, k), 10 ** 9, dtype=torch.int64, device='cuda')
    hip.topk_chunk(part_val, 0, k, val, idx, 0, ids_in=part_idx)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_S.cpu().numpy()), bits(S))
    bad = first_bad_row(val.cpu().numpy(), idx.cpu().numpy(), ref_val, ref_idx)
    assert bad is None, (N, C, k, 'row', bad, idx[bad].tolist(), ref_idx[bad].tolist())


# ---------------------------------------------------------------------------
# 5. more rows than the capped grid serves in one sweep
# ---------------------------------------------------------------------------
def grid_cap_rows(B):
    """Quantised rows of 70 columns with row i's unique maximum at column i % 70: a row served by the wrong iteration of
    the grid-stride loop shows in its first id."""
    rng = np.random.default_rng(B)
    S = (rng.integers(-4, 4, (B, 70)) / 8.0).astype(np.float32)
    S[np.arange(B), np.arange(B) % 70] = 1.0
    return S


@pytest.mark.parametrize('filtered', [False, True], ids=['plain', 'targets'])
def test_one_pass_kernel_past_the_grid_cap(hip, filtered):
    """B = 16384 + 5 rows, four per block and 4096 blocks: the second sweep has two blocks, the last with one active
    wave.  With targets: one per row, the row's maximum for odd rows."""
    B, k, c_base = 16384 + 5, 8, 1000
    S = grid_cap_rows(B)
    masked, seg = S, None
    if filtered:
        col = np.where(np.arange(B) % 2 == 1, np.arange(B) % 70, (np.arange(B) + 13) % 70)
        perm = np.random.default_rng(5).permutation(B)              # the segments lie in no particular order
        targets = np.empty(B, np.int32)
        targets[perm] = (col + c_base).astype(np.int32)
        seg = (perm.astype(np.int64), perm.astype(np.int64) + 1, targets)
        masked = S.copy()
        masked[np.arange(B), col] = -INF
    ref_val, ref_idx = reference(masked, k, c_base=c_base)
    val, idx = run_chunk(hip, S, k, c_base, seg=seg, expect_tile=masked)
    bad = first_bad_row(val, idx, ref_val, ref_idx)
    assert bad is None, ('row', bad, idx[bad].tolist(), ref_idx[bad].tolist())


def test_fallback_kernel_past_the_grid_cap(hip):
    B, k = 4096 + 3, 33
    S = grid_cap_rows(B)
    ref_val, ref_idx = reference(S, k, c_base=1000)
    val, idx = run_chunk(hip, S, k, 1000)
    bad = first_bad_row(val, idx, ref_val, ref_idx)
    assert bad is None, ('row', bad, idx[bad].tolist(), ref_idx[bad].tolist())


def test_kge_topk_past_the_grid_cap(hip):
    B, k = 4096 + 3, 3
    S = grid_cap_rows(B)
    ref_val, ref_idx = reference(S, k)
    val, idx = hip.topk(torch.from_numpy(S).cuda(), k)
    bad = first_bad_row(val.cpu().numpy(), idx.cpu().numpy(), ref_val, ref_idx)
    assert bad is None, ('row', bad, idx[bad].tolist(), ref_idx[bad].tolist())


# ---------------------------------------------------------------------------
# 6. refusals and the empty batch
# ---------------------------------------------------------------------------
def test_error_codes_and_empty_batch_write_nothing(hip):
    lib = hip.load_library()
    B, C, k, ld, ldo = 4, 100, 8, 104, COL_OFF + 8 + 2
    S = torch.from_numpy(family_matrix(C, k, ['normal', 'quantised', 'specials', 'constant']))
    tile = carve(S, ld - C, 0, INF, device='cuda')
    lo = torch.zeros(B, dtype=torch.int64, device='cuda')
    hi = torch.ones(B, dtype=torch.int64, device='cuda')
    tg = torch.full((B,), 5, dtype=torch.int32, device='cuda')
    ids = torch.arange(C, dtype=torch.int64, device='cuda').repeat(B, 1)
    out_idx, out_val = guarded_out(B, ldo, 0, 0, dtype=torch.int64), guarded_out(B, ldo, 0, 0)

    def call(B=B, C=C, ld=ld, k=k, lo=lo, hi=hi, tg=tg, ids=None, ld_ids=0, ldo=ldo, col_off=COL_OFF):
        return raw(lib, 'kge_topk_chunk', tile, ld, B, C, 0, k, lo, hi, tg, ids, ld_ids, out_idx, out_val, ldo, col_off)
    assert call(C=0) == KGE_EINVAL
    assert call(ld=C - 1) == KGE_EINVAL
    assert call(k=0) == KGE_EINVAL
    assert call(ldo=COL_OFF + k - 1) == KGE_EINVAL
    assert call(lo=None) == KGE_EINVAL                              # targets without seg_lo
    assert call(ids=ids, ld_ids=C - 1) == KGE_EINVAL
    assert call(B=0) == 0
    assert call(B=0, ids=ids, ld_ids=C) == 0
    assert raw(lib, 'kge_topk', tile, ld, 0, C, k, out_idx, out_val) == 0
    torch.cuda.synchronize()
    assert_guard_intact(out_idx, rows=0)                            # every element still holds its sentinel
    assert_guard_intact(out_val, rows=0)
    assert_guard_intact(tile)
    assert np.array_equal(bits(tile.cpu().numpy()), bits(S.numpy()))
    assert call() == 0 and call(ids=ids, ld_ids=C) == 0             # (the same arguments are accepted when legal)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 7. the switch: KGE_TOPK_REG=0 sends k <= 32 to the k-pass kernel
# ---------------------------------------------------------------------------
CHILD = ('import sys; sys.path.insert(0, sys.argv[1]); '
         'from tests.test_gpu_topk_kernels import switch_child; switch_child(sys.argv[2])')


def switch_child(path):
    """Body of the child process: the SWITCH_CASES launches of the first test, saved as one .npz."""
    from torchkge_amd import _hip
    _hip.load_library()
    out = {}
    for C, k in SWITCH_CASES:
        val, idx = run_chunk(_hip, family_matrix(C, k), k, 1000)
        out['val_%d_%d' % (C, k)], out['idx_%d_%d' % (C, k)] = val, idx
    np.savez(path, **out)


@pytest.fixture(scope='module')
def fallback_child(hip, tmp_path_factory):
    """One fresh child process (never an exec of this one) with KGE_TOPK_REG=0 in its environment.  An abnormal exit
    fails every test that uses it, and nothing more is run for them."""
    path = str(tmp_path_factory.mktemp('topk_switch') / 'fallback.npz')
    env = dict(os.environ, KGE_TOPK_REG='0')
    r = subprocess.run([sys.executable, '-c', CHILD, ROOT, path], env=env, cwd=ROOT, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, 'the KGE_TOPK_REG=0 child ended with %r:\n%s' % (r.returncode, r.stdout[-4000:])
    with np.load(path) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize('C,k', SWITCH_CASES, ids=['C%d-k%d' % ck for ck in SWITCH_CASES])
def test_switch_to_the_fallback_gives_the_same_bits(hip, fallback_child, C, k):
    val, idx, ref_val, ref_idx = family_launch(hip, 'chunk', C, k)
    f_val, f_idx = fallback_child['val_%d_%d' % (C, k)], fallback_child['idx_%d_%d' % (C, k)]
    bad = first_bad_row(f_val, f_idx, ref_val, ref_idx)
    assert bad is None, (C, k, FAMILIES[bad], 'fallback vs reference', f_idx[bad].tolist(), ref_idx[bad].tolist())
    bad = first_bad_row(f_val, f_idx, val, idx)
    assert bad is None, (C, k, FAMILIES[bad], 'fallback vs one-pass', f_idx[bad].tolist(), idx[bad].tolist())
