"""GPU tests of kge_row_penalty / kge_row_penalty_bwd (include/kge_hip_penalty.h) through the C entries, against the
float64 yardstick of tests/penalty_ref.py.

The bounds are derived, with u = 2 ** -24 and tables of O(1) magnitude (nothing subnormal).  All terms are non-negative:
no cancellation.
  terms   at most 6 roundings per element term (complex, p = 3: re * re, the fmaf, sqrtf, m2 * m -- 4; the bound allows
          6), 2 additions inside a group, ceil(d / 256) additions into the lane accumulator (lane l owns the groups
          l, l + 64, ...: one per 256 floats), 6 butterfly steps, 1 for the factor:
          |terms - ref| <= (16 + ceil(d / 256)) u ref.
  rows    p * factor, times go, m2 in two roundings, sqrtf, c * m, times the element: 7, the bound allows 8:
          |got - ref| <= 8 u |ref| element by element.
  loss    the fp64 tree adds M fp32 terms with a relative error of M * 2 ** -53 -- far below half an fp32 ulp -- and
          rounds once: within 1 ulp of the float64 sum of the GPU's own terms, rounded to fp32."""
import ctypes
import math

import pytest
import torch

from tests import penalty_ref as ref
from tests.helpers import carve, guarded_out, assert_guard_intact, raw

from torchkge_amd import _hip_penalty as hp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LAYOUTS = [hp.REAL, hp.SPLIT, hp.INTERLEAVED]
WIDTHS = [1, 2, 3, 5, 64, 66, 200, 254, 256, 258, 1030]
ROWS = 40


def widths(layout):
    return [d for d in WIDTHS if layout != hp.INTERLEAVED or d % 2 == 0]


def table(rows, d, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(rows, d, generator=g) * 1.5 + 0.25) * (torch.randint(0, 2, (rows, d), generator=g) * 2 - 1) * scale).cuda()


def stream(layout, d, n, seed, rows=ROWS, factor=None, ids=None, scale=1.0):
    """One stream tuple (layout, t0, t1, ids, factor) on the GPU: O(1) entries of both signs, ids with repeats."""
    t0 = table(rows, d, seed, scale)
    t1 = table(rows, d, seed + 1000, scale) if layout == hp.SPLIT else None
    if ids is None:
        ids = torch.randint(0, rows, (n,), generator=torch.Generator().manual_seed(seed + 7)).cuda()
    return (layout, t0, t1, ids, (0.3 / max(n, 1)) if factor is None else factor)


def run(streams, p, go=1.0, off_terms=0, off_rows=0, acc=None, backward=True):
    """Both entries on sentinel-filled outputs: (terms, loss, rows); nothing outside the M terms and the rows buffer may
    have been written."""
    lib = hp.load_library()
    arr, keep = hp.descriptors(streams)
    n = len(streams)
    M, floats = hp.n_terms(arr, n), hp.row_offsets(arr, n)[-1]
    terms = guarded_out(max(M, 1), off=off_terms)       # (an empty tensor has no address: one guarded element instead)
    loss = guarded_out(1)
    ws = torch.empty(max(int(lib.kge_row_penalty_ws_bytes(M)), 16), dtype=torch.uint8, device='cuda')
    assert raw(lib, 'kge_row_penalty', arr, n, p, terms, loss, acc, ws, ws.numel()) == 0
    assert_guard_intact(terms, rows=M)
    assert_guard_intact(loss)
    rows = None
    if backward:
        rows = guarded_out(max(floats, 1), off=off_rows)
        g = torch.tensor([go], dtype=torch.float32, device='cuda')
        assert raw(lib, 'kge_row_penalty_bwd', arr, n, p, g, rows) == 0
        assert_guard_intact(rows, rows=floats)
    return terms[:M].clone(), loss.clone()[0], (None if rows is None else rows[:floats].clone())


def cpu(streams):
    return [(layout, t0.cpu(), None if t1 is None else t1.cpu(), ids.cpu(), f) for layout, t0, t1, ids, f in streams]


def check(streams, p, terms, rows, go=1.0):
    """The derived bounds of the module docstring, per stream (its own d)."""
    want_t, want_r = ref.terms(cpu(streams), p), ref.gradient_rows(cpu(streams), p, float(torch.tensor(go, dtype=torch.float32)))
    terms, rows = terms.cpu().double(), rows.cpu().double()
    assert terms.shape == want_t.shape and rows.shape == want_r.shape
    at = 0
    for layout, t0, t1, ids, f in streams:
        n, d = ids.shape[0], t0.shape[1]
        bound = (16 + math.ceil(d / 256)) * U * want_t[at:at + n]
        err = (terms[at:at + n] - want_t[at:at + n]).abs()
        assert bool((err <= bound).all()), (layout, p, d, n, float((err / want_t[at:at + n]).max() / U))
        at += n
    err = (rows - want_r).abs()
    assert bool((err <= 8 * U * want_r.abs()).all()), (p, float((err / want_r.abs().clamp_min(1e-300)).max() / U))
    assert bool(torch.isfinite(terms).all()) and bool(torch.isfinite(rows).all())


def check_loss(terms, loss, acc_before=None, acc_after=None):
    want = terms.double().sum().float()
    ulp = torch.nextafter(want, want * 2) - want
    assert abs(float(loss) - float(want)) <= float(ulp), (float(loss), float(want))
    if acc_before is not None:
        assert float(acc_after) == float(torch.tensor(acc_before, dtype=torch.float32) + loss.cpu())


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('p', [2, 3])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_every_width_and_batch_size_within_the_derived_bounds(layout, p):
    """d: one group, a ragged last group, exactly one pass of the 64 lanes' quads (256), one past it, several passes;
    n: one row, one id for every row (7 of 7, each once), 300 with repeats."""
    for d in widths(layout):
        for n in (1, 7, 300):
            if n == 7:
                s = stream(layout, d, n, seed=d + n, rows=7, ids=torch.randperm(7, generator=torch.Generator().manual_seed(d)).cuda())
            else:
                s = stream(layout, d, n, seed=d + n)
            go = 1.0 if n == 1 else 0.37
            terms, loss, rows = run([s], p, go=go)
            check([s], p, terms, rows, go=go)
            check_loss(terms, loss)


@pytest.mark.parametrize('p', [2, 3])
def test_several_streams_of_mixed_layouts_and_widths_in_one_call(p):
    """1, 3 and 8 streams; a stream of no rows among them; every row's term and gradient rows carry the bits they have
    when their stream is the only one of the call."""
    mix = [stream(hp.REAL, 5, 7, 1), stream(hp.SPLIT, 66, 30, 2), stream(hp.INTERLEAVED, 258, 9, 3), stream(hp.REAL, 1030, 4, 4),
           stream(hp.SPLIT, 3, 0, 5), stream(hp.INTERLEAVED, 2, 300, 6), stream(hp.REAL, 256, 1, 7), stream(hp.SPLIT, 200, 11, 8)]
    for count in (1, 3, 8):
        streams = mix[:count]
        terms, loss, rows = run(streams, p, go=0.5)
        check(streams, p, terms, rows, go=0.5)
        check_loss(terms, loss)
        alone_t, alone_r = [], []
        for s in streams:
            t, _, r = run([s], p, go=0.5)
            alone_t.append(t)
            alone_r.append(r)
        assert same_bits(terms, torch.cat(alone_t)) and same_bits(rows, torch.cat(alone_r))


def test_beyond_the_grid_cap_the_wavefronts_stride():
    """M = KGE_PENALTY_MAX_BLOCKS * KGE_PENALTY_WAVES + 3 rows at d = 5: every wavefront takes a second row, three a
    third; the sum takes its second stage (M > KGE_PAIR_LOSS_CHUNK = 1024 terms per block: three launches)."""
    M = hp.MAX_BLOCKS * hp.WAVES + 3
    s = stream(hp.REAL, 5, M, seed=11, rows=100)
    acc = torch.tensor([1.5], dtype=torch.float32, device='cuda')
    terms, loss, rows = run([s], 3, go=2.0, acc=acc)
    check([s], 3, terms, rows, go=2.0)
    check_loss(terms, loss, 1.5, acc[0].cpu())
    assert int(hp.load_library().kge_row_penalty_ws_bytes(M)) > 8


@pytest.mark.parametrize('p', [2, 3])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_load_path_alignment_and_padding_do_not_change_a_bit(layout, p):
    """A table one float off a 16-byte boundary, a leading dimension above d with NaN-poisoned pads, outputs one float
    off: the bits of the aligned contiguous call; and a second call repeats the first."""
    for d in (6, 64, 258):
        base = stream(layout, d, 33, seed=d)
        terms, loss, rows = run([base], p, go=0.7)
        again = run([base], p, go=0.7)
        assert same_bits(terms, again[0]) and same_bits(rows, again[2]) and same_bits(loss.view(1), again[1].view(1))
        _, t0, t1, ids, f = base
        for pad, off in ((0, 1), (2, 0), (3, 0), (4, 0), (5, 3)):      # (leading dimensions on and off a multiple of four)
            moved = (layout, carve(t0, pad=pad, off=off), None if t1 is None else carve(t1, pad=pad, off=off), ids, f)
            assert moved[1].data_ptr() % 16 == 4 * off and moved[1].stride(0) == d + pad
            got = run([moved], p, go=0.7, off_terms=off, off_rows=off)
            assert same_bits(terms, got[0]) and same_bits(rows, got[2]) and same_bits(loss.view(1), got[1].view(1)), (d, pad, off)
            assert_guard_intact(moved[1])


@pytest.mark.parametrize('p', [2, 3])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_a_rows_term_does_not_depend_on_its_batch(layout, p):
    s = stream(layout, 66, 50, seed=3)
    terms, _, rows = run([s], p)
    _, t0, t1, ids, f = s
    d = 66
    for i in (0, 17, 49):
        one = (layout, t0, t1, ids[i:i + 1].clone(), f)
        t, _, r = run([one], p)
        assert same_bits(t, terms[i:i + 1])
        if layout == hp.SPLIT:
            assert same_bits(r[:d], rows[i * d:(i + 1) * d]) and same_bits(r[d:], rows[(50 + i) * d:(51 + i) * d])
        else:
            assert same_bits(r, rows[i * d:(i + 1) * d])


@pytest.mark.parametrize('p', [2, 3])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_zero_rows_and_zero_coordinates_give_bit_zero_terms_and_gradients(layout, p):
    """No division anywhere: row 0 is all zero, row 1 has zero coordinates among non-zero ones."""
    for d in (6, 258):
        layout_, t0, t1, _, f = stream(layout, d, 1, seed=9)
        t0[0] = 0
        step = 2 if layout == hp.INTERLEAVED else 1
        for k in (0, 2 * step):         # a whole coordinate: both floats of an interleaved pair, both tables of a SPLIT one
            t0[1, k:k + step] = 0
        if t1 is not None:
            t1[0] = 0
            t1[1, 0] = 0
            t1[1, 2] = 0
        ids = torch.tensor([0, 1, 0], device='cuda')
        s = (layout, t0, t1, ids, f)
        terms, loss, rows = run([s], p, go=1.25)
        check([s], p, terms, rows, go=1.25)
        assert not bool(torch.isnan(rows).any())
        assert int(terms.view(torch.int32)[0]) == 0 and int(terms.view(torch.int32)[2]) == 0 and float(terms[1]) > 0
        blocks = rows.view(-1, 3, d)        # (blocks, rows, d)
        assert bool((blocks[:, 0].view(torch.int32) == 0).all()) and bool((blocks[:, 2].view(torch.int32) == 0).all())
        zero_cols = [0, 1, 4, 5] if layout == hp.INTERLEAVED else [0, 2]
        assert bool((blocks[:, 1, zero_cols].view(torch.int32) == 0).all())
        assert int((blocks[:, 1] != 0).sum()) == blocks.shape[0] * (d - len(zero_cols))


@pytest.mark.parametrize('p', [2, 3])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_rows_of_magnitude_1e6_stay_finite_within_the_same_relative_bound(layout, p):
    s = stream(layout, 258, 20, seed=13, scale=1e6)
    terms, loss, rows = run([s], p, go=1.0)
    check([s], p, terms, rows)
    check_loss(terms, loss)
    assert math.isfinite(float(loss))


def test_an_empty_batch_writes_a_zero_loss_and_leaves_the_accumulator():
    lib = hp.load_library()
    s = stream(hp.REAL, 8, 0, seed=1)
    acc = torch.tensor([2.5], dtype=torch.float32, device='cuda')
    terms, loss, rows = run([s], 3, acc=acc)
    assert float(loss) == 0.0 and float(acc[0]) == 2.5 and terms.numel() == 0 and rows.numel() == 0
    out = guarded_out(1)
    assert raw(lib, 'kge_row_penalty', None, 0, 2, guarded_out(1), out, None, None, 0) == 0
    assert float(out[0]) == 0.0
    # acc_io gains exactly the loss, twice in a row
    s = stream(hp.SPLIT, 64, 10, seed=2)
    _, l1, _ = run([s], 3, acc=acc, backward=False)
    _, l2, _ = run([s], 3, acc=acc, backward=False)
    want = (torch.tensor(2.5) + l1.cpu()) + l2.cpu()
    assert float(acc[0]) == float(want) and same_bits(l1.view(1), l2.view(1))


def test_the_binding_returns_what_the_entries_write():
    streams = [stream(hp.SPLIT, 66, 30, 2), stream(hp.REAL, 5, 7, 1)]
    terms, loss, rows = run(streams, 3, go=0.5)
    acc = torch.zeros((), dtype=torch.float32, device='cuda')
    got_loss, got_terms = hp.row_penalty(streams, 3, acc)
    got_rows, offs = hp.row_penalty_bwd(streams, 3, torch.tensor(0.5, device='cuda'))
    assert same_bits(got_terms, terms) and same_bits(got_loss.view(1), loss.view(1)) and same_bits(got_rows, rows)
    assert float(acc) == float(loss) and offs == [0, 2 * 30 * 66, 2 * 30 * 66 + 35]
