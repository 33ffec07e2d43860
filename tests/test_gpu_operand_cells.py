# -*- coding: utf-8 -*-
"""The BYTES of the f16 operands of the split prefilter: every writer against the numpy model of tests/operand_ref.py.

The other GPU modules compare the writers with each other (the fused pipelines against the separate kernels); a change
made consistently in all of them would pass there.  Here the split operand, the planar and the fragment-major hi operand,
the augmentation columns of aug modes 0..4, the padding rows, the operand scales, the guard column, cell_ss, the row_index
gather and the per-query scales of the DOT pipeline are pinned byte for byte, the residuals (any-order fp32 sums) within
the bounds the parity tests use for them.  Shapes are the smallest that reach each branch of each writer.

Wherever a scale is derived from a norm the inputs are chosen so that log2(16384 / sqrt(norm^2)) lies at least 0.05 away
from an integer (asserted): the device's log2f then cannot land in another binade than numpy's."""
import ctypes
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import operand_ref as ref
from tests.helpers import oracle_clib, fptr, carve, raw

pytestmark = pytest.mark.gpu
F = np.float32
f = ctypes.c_float
K_LIST = [4, 15, 16, 17, 264]       # float4 path, scalar path, the augmentation column alone in its unit, a second tile of 16 units


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


def _rows(seed, rows, K, amp=1.0):
    """Rows of norm about `amp` whose values spread over two decades (hi parts of every exponent, non-zero lo parts)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, K)) * 10.0 ** rng.uniform(-2, 0, size=(rows, K))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return np.ascontiguousarray((X * amp * rng.uniform(0.5, 1.0, size=(rows, 1))).astype(F))


def _sq(X):
    return (X.astype(np.float64) ** 2).sum(axis=1)


def _safe_bound(n):
    """A squared-norm bound >= n that sits in the middle of its scale's binade."""
    fr = float(ref.scale_log2_frac(n))
    m = np.sqrt(float(n)) * 2.0 ** (fr - 0.5 if fr >= 0.5 else fr + 0.5)
    out = F(m * m)
    assert out >= n and ref.scale_is_safe(out)
    return out


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bytes(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint8).reshape(-1)


def _assert_bound(got, model, what):
    """An any-order fp32 sum against its float64 model: within rtol 3e-4 and never below it by more than 1e-5."""
    got, model = np.asarray(got, dtype=np.float64), np.asarray(model, dtype=np.float64)
    assert np.all(np.abs(got - model) <= 3e-4 * model), what
    assert np.all(got >= model * (1 - 1e-5)), what


def _mode_args(mode, X0, X1):
    """(aug, aug_mul, nmax, scale) of an aug mode: the L2 modes on the fixed scale, the DOT modes on a norm bound."""
    n = _sq(X0) + (0 if X1 is None else _sq(X1))
    if mode in (3, 4):
        nmax = _safe_bound(n.max())
        return (n.astype(F) if mode == 3 else None), (1.0 if mode == 3 else 0.0), nmax, ref.split_scale(nmax)
    return (n.astype(F) if mode == 1 else None), {0: 0.0, 1: -0.5, 2: 1.0}[mode], None, ref.FIXED_SCALE


def _split_case(lib, X0, X1, is_query, mode, idx=None, pad=0, off=0, want_css=True):
    """One kge_lp_split_rows call on [X0 | X1] (rows gathered by idx) against the model: bytes, cell_ss."""
    K0, K1 = X0.shape[1], 0 if X1 is None else X1.shape[1]
    aug, aug_mul, nmax, scale = _mode_args(mode, X0, X1)
    G0, G1, gaug = (X0, X1, aug) if idx is None else (X0[idx], None if X1 is None else X1[idx], None if aug is None else aug[idx])
    rows = G0.shape[0]
    rows_p = int(lib.kge_lp_split_rows_padded(rows, is_query))
    units_p = int(lib.kge_lp_split_units(K0 + K1, 1 if mode else 0))
    d0 = carve(torch.from_numpy(X0), pad, off, device='cuda')
    d1 = None if X1 is None else carve(torch.from_numpy(X1), pad, off, device='cuda')
    out = torch.full((rows_p * units_p * 64,), 0xA5, dtype=torch.uint8, device='cuda')
    css = torch.full((units_p * rows_p,), float('nan'), device='cuda') if want_css else None
    d_n = None if nmax is None else _dev(np.array([nmax, 0.0], F))
    assert raw(lib, 'kge_lp_split_rows', d0, K0 + pad, K0, d1, K1 + pad if K1 else 0, K1, rows, is_query, mode, _dev(aug), f(aug_mul),
               d_n, None if d_n is None else d_n[1:], out, css, _dev(idx)) == 0
    hi, lo = ref.split_values(G0, G1, rows_p, units_p, mode, gaug, aug_mul, scale, 0.0 if nmax is None else nmax)
    key = (K0, K1, rows, is_query, mode, pad, off)
    assert np.array_equal(_bytes(out), ref.split_bytes(hi, lo)), key
    if want_css:
        want = ref.cell_ss(G0, G1, rows_p, units_p)
        got = css.cpu().numpy().astype(np.float64).reshape(units_p, rows_p)
        assert np.all(np.abs(got - want) <= 1e-6 * want), key


@pytest.mark.parametrize('K', K_LIST)
def test_split_rows_bytes_every_mode_and_role(hip, K):
    """kge_lp_split_rows: one and 257 rows, as candidates (256-row padding) and as queries (192), aug modes 0..4."""
    lib = hip.load_library()
    for rows in (1, 257):
        X = _rows(K * 7 + rows, rows, K, amp=1.0)
        Xd = _rows(K * 7 + rows + 1, rows, K, amp=3.0)
        for is_query, mode in itertools.product((0, 1), range(5)):
            _split_case(lib, Xd if mode in (3, 4) else X, None, is_query, mode)


def test_split_rows_bytes_across_the_segment_seam_gathered_strided_and_unaligned(hip):
    """Two segments of 40 columns (the cell of columns 32..47 straddles the seam), a row_index gather, a row stride of
    K + 4 floats, and a base one float off a 16-byte boundary (scalar loads)."""
    lib = hip.load_library()
    X0, X1 = _rows(1, 257, 40, 2.0), _rows(2, 257, 40, 1.5)
    for mode in (3, 4, 0):
        _split_case(lib, X0, X1, 1 if mode == 3 else 0, mode)
    idx = np.random.default_rng(3).integers(0, 257, 70).astype(np.int64)
    _split_case(lib, X0, X1, 1, 3, idx=idx)
    _split_case(lib, _rows(4, 257, 17), None, 0, 1, idx=idx)
    for K in (16, 264):
        _split_case(lib, _rows(5, 33, K), None, 0, 1, pad=4)
        _split_case(lib, _rows(6, 33, K), None, 1, 2, off=1)


@pytest.mark.parametrize('K', K_LIST)
def test_hi_rows_bytes_planar_and_fragment_major(hip, K):
    """kge_lp_hi_rows / kge_lp_hi_rows_frag, aug modes 1..4: 33 rows (a partial 32-row group) and 257 (a second candidate
    tile); the table byte for byte, dn2 and dn2max as bounds."""
    lib = hip.load_library()
    units_p = int(lib.kge_lp_hi_units(K))
    for rows, mode, frag in itertools.product((33, 257), (1, 2, 3, 4), (0, 1)):
        X = _rows(K * 11 + rows + mode, rows, K, amp=3.0 if mode in (3, 4) else 1.0)
        aug, aug_mul, nmax, scale = _mode_args(mode, X, None)
        is_query = 0 if frag else int(mode in (2, 3))
        rows_p = int(lib.kge_lp_split_rows_padded(rows, is_query))
        out = torch.full((rows_p * units_p * 32,), 0xA5, dtype=torch.uint8, device='cuda')
        dn2, dmx = torch.full((rows,), float('nan'), device='cuda'), torch.zeros(1, device='cuda')
        d_n = None if nmax is None else _dev(np.array([nmax], F))
        head = (_dev(X), K, K, None, 0, 0, rows)
        tail = (mode, _dev(aug), f(aug_mul), d_n, None, out, dn2, dmx)
        if frag:
            assert raw(lib, 'kge_lp_hi_rows_frag', *head, *tail) == 0
        else:
            assert raw(lib, 'kge_lp_hi_rows', *head, is_query, *tail, None) == 0
        hi = ref.hi_values(X, None, rows_p, units_p, mode, aug, aug_mul, scale, 0.0 if nmax is None else nmax)
        key = (K, rows, mode, frag)
        assert np.array_equal(_bytes(out), ref.frag_bytes(hi) if frag else ref.planar_bytes(hi)), key
        want = ref.residuals(X, None, scale)
        _assert_bound(dn2.cpu().numpy(), want, key)
        _assert_bound(dmx.cpu().numpy(), want.max(), key)


def test_hi_rows_bytes_two_segments_and_gather(hip):
    """The planar writer across a segment seam inside a cell, with a row_index gather (query columns of a DOT problem)."""
    lib = hip.load_library()
    X0, X1 = _rows(21, 90, 40, 2.0), _rows(22, 90, 40, 1.5)
    idx = np.random.default_rng(23).integers(0, 90, 33).astype(np.int64)
    aug, aug_mul, nmax, scale = _mode_args(3, X0, X1)
    rows_p, units_p = int(lib.kge_lp_split_rows_padded(33, 1)), int(lib.kge_lp_hi_units(80))
    out = torch.full((rows_p * units_p * 32,), 0xA5, dtype=torch.uint8, device='cuda')
    dn2 = torch.full((33,), float('nan'), device='cuda')
    d_n = _dev(np.array([nmax, 0.0], F))
    assert raw(lib, 'kge_lp_hi_rows', _dev(X0), 40, 40, _dev(X1), 40, 40, 33, 1, 3, _dev(aug), f(aug_mul), d_n, d_n[1:], out, dn2,
               None, _dev(idx)) == 0
    hi = ref.hi_values(X0[idx], X1[idx], rows_p, units_p, 3, aug[idx], aug_mul, scale, nmax)
    assert np.array_equal(_bytes(out), ref.planar_bytes(hi))
    _assert_bound(dn2.cpu().numpy(), ref.residuals(X0[idx], X1[idx], scale), 'dn2')


def _dot_table(K0, K1, rows):
    """A DOT candidate table whose segments' squared-norm maxima ask for a scale well inside its binade."""
    X0 = _rows(K0 + rows, rows, K0, 2.0)
    X1 = _rows(K0 + rows + 1, rows, K1, 1.5) if K1 else None
    for _ in range(2):          # (rescale the whole table; the second pass absorbs the fp32 rounding of the first)
        n = F(_sq(X0).max()) + (F(_sq(X1).max()) if K1 else F(0))
        c = F(np.sqrt(_safe_bound(n) / n))
        X0 = (X0 * c).astype(F)
        X1 = (X1 * c).astype(F) if K1 else None
    return X0, X1


@pytest.mark.parametrize('K0,K1', [(8, 0), (136, 136)])
@pytest.mark.parametrize('rows', [33, 257])
def test_dot_table_prep_bytes_two_launches_and_fused(hip, K0, K1, rows):
    """kge_lp_dot_table_prep / _fused on float4-readable rows (the coalesced kernel): one span, and two spans of 256 columns
    with the segment seam inside the first; the fragment-major table byte for byte, the squared-norm maxima and the
    residual block maxima as bounds."""
    lib = hip.load_library()
    X0, X1 = _dot_table(K0, K1, rows)
    n0, n1 = _sq(X0).max(), (_sq(X1).max() if K1 else 0.0)
    nmax = F(n0) + F(n1)
    assert ref.scale_is_safe(nmax)
    scale = ref.split_scale(nmax)
    rows_p, units_p = int(lib.kge_lp_split_rows_padded(rows, 0)), int(lib.kge_lp_hi_units(K0 + K1))
    want = ref.frag_bytes(ref.hi_values(X0, X1, rows_p, units_p, 4, scale=scale))
    resid = ref.residuals(X0, X1, scale).max()
    nb0, nb1 = int(lib.kge_lp_dot_table_prep_blocks(rows, 0)), int(lib.kge_lp_dot_table_prep_blocks(rows, 1))
    d0, d1 = _dev(X0), _dev(X1)
    # two launches: the maxima measured first
    out = torch.full((rows_p * units_p * 32,), 0xA5, dtype=torch.uint8, device='cuda')
    nm, dnb, ws = torch.zeros(2, device='cuda'), torch.full((nb1,), float('nan'), device='cuda'), torch.empty(2 * nb0, device='cuda')
    assert raw(lib, 'kge_lp_dot_table_prep', d0, K0, K0, d1, K1, K1, rows, 1, nm[0:1], nm[1:2] if K1 else None, out, dnb, ws) == 0
    assert np.array_equal(_bytes(out), want)
    _assert_bound(nm.cpu().numpy()[:2 if K1 else 1], [n0, n1][:2 if K1 else 1], 'norm maxima')
    _assert_bound(dnb.cpu().numpy().max(), resid, 'residual block maxima')
    # one launch: the scale of the maxima a previous evaluation left
    out = torch.full((rows_p * units_p * 32,), 0xA5, dtype=torch.uint8, device='cuda')
    dnb, nmb = torch.full((nb1,), float('nan'), device='cuda'), torch.full((2 * nb1,), float('nan'), device='cuda')
    assert raw(lib, 'kge_lp_dot_table_prep_fused', d0, K0, K0, d1, K1, K1, rows, _dev(np.array([n0, n1], F)), out, dnb, nmb) == 0
    assert np.array_equal(_bytes(out), want)
    got = nmb.cpu().numpy().reshape(2, nb1).max(axis=1)
    _assert_bound(got[:2 if K1 else 1], [n0, n1][:2 if K1 else 1], 'fused norm maxima')
    assert K1 or got[1] == 0.0
    _assert_bound(dnb.cpu().numpy().max(), resid, 'fused residual block maxima')


@pytest.mark.parametrize('K', [4, 12, 16, 200, 264])
@pytest.mark.parametrize('N', [5, 257])
def test_table_prep_l2_bytes(hip, K, N):
    """kge_lp_table_prep_l2: en bit for bit the sequential fmaf chain, the fragment-major table byte for byte (data tail and
    both augmentation columns in one unit, the columns alone in theirs, padding rows), the maxima."""
    lib = hip.load_library()
    E = _rows(K * 3 + N, N, K, 1.3)
    en = np.empty(N, F)
    i64 = ctypes.c_int64
    oracle_clib().orc_row_sqnorm_chain(fptr(E), i64(K), i64(N), i64(K), fptr(en))
    rows_p, units_p = int(lib.kge_lp_split_rows_padded(N, 0)), int(lib.kge_lp_hi_units(K))
    d_en, mx = torch.full((N,), float('nan'), device='cuda'), torch.zeros(2, device='cuda')
    out = torch.full((rows_p * units_p * 32,), 0xA5, dtype=torch.uint8, device='cuda')
    assert raw(lib, 'kge_lp_table_prep_l2', _dev(E), K, N, K, d_en, mx[0:1], out, mx[1:2], None) == 0
    got_en = d_en.cpu().numpy()
    assert np.array_equal(got_en.view(np.uint32), en.view(np.uint32))
    hi = ref.hi_values(E, None, rows_p, units_p, 1, en, -0.5)
    assert np.array_equal(_bytes(out), ref.frag_bytes(hi))
    assert mx.cpu().numpy()[0] == en.max()
    _assert_bound(mx.cpu().numpy()[1], ref.residuals(E, None, safety=1.0002).max(), 'dn2max')


def _facts(rng, n_ent, n_rel, B):
    return rng.integers(0, n_ent, B), rng.integers(0, n_ent, B), rng.integers(0, n_rel, B)


@pytest.mark.parametrize('level', [0, 1])
@pytest.mark.parametrize('d', [8, 40, 52, 200])
def test_query_pipeline_operand_bytes(hip, level, d):
    """kge_lp_query_pipeline, both sides of 5 facts: less than one 48-column chunk, a chunk edge inside a unit (d = 40: the
    augmentation columns; 52: data), several chunks.  Qs byte for byte from the kernel's own Q; at d = 40 also per column."""
    lib = hip.load_library()
    rng = np.random.default_rng(100 * d + level)
    E, R = _rows(d, 50, d, 1.0), _rows(d + 1, 7, d, 0.4)
    h, t, r = _facts(rng, 50, 7, 5)
    dE, dR = _dev(E), _dev(R)
    en = hip.row_sqnorm(dE)
    emax, qmax, de2 = en.max().view(1).clone(), torch.zeros(1, device='cuda'), torch.full((1,), 1e-7, device='cuda')
    Bp = int(lib.kge_lp_split_rows_padded(10, 1))
    units_p = int(lib.kge_lp_hi_units(d)) if level else int(lib.kge_lp_split_units(d, 1))
    plans = [None]
    if d == 40:
        qs_row = torch.tensor([3, -1, 0, 7, 1, -1, 2, 9, 4, 5], dtype=torch.int32, device='cuda')
        plans.append(SimpleNamespace(n_single_p=Bp, n_multi_p=0, n_queries=10, qs_row=qs_row))
    for cols in plans:
        out = hip.lp_query_pipeline(hip.SIDE_BOTH, dE, dR, _dev(h), _dev(t), _dev(r), en, emax, qmax, level=level,
                                    de2max=de2 if level else None, cols=cols)
        torch.cuda.synchronize()
        Q = out['Q'].cpu().numpy()
        assert np.array_equal(Q, np.concatenate([E[h] + R[r], E[t] - R[r]]))
        if level:
            want = ref.planar_bytes(ref.hi_values(Q, None, Bp, units_p, 2, aug_mul=1.0))
            _assert_bound(out['q_dn2'].cpu().numpy(), ref.residuals(Q, None), 'q_dn2')
        else:
            want = ref.split_bytes(*ref.split_values(Q, None, Bp, units_p, 2, aug_mul=1.0))
        got, want = _bytes(out['Qs']).reshape(Bp, -1), want.reshape(Bp, -1)
        if cols is None:
            assert np.array_equal(got, want), (level, d)
        else:
            for q, row in enumerate(cols.qs_row.cpu().tolist()):
                assert row < 0 or np.array_equal(got[row], want[q]), (level, d, q)


def _dot_queries(d, cplx):
    """Tables and 5 facts of a DistMult / ComplEx batch whose 10 query rows each ask for a scale well inside its binade."""
    for seed in range(10000):
        rng = np.random.default_rng(977 * d + seed)
        tabs = [_rows(rng.integers(1 << 30), n, d, a) for n, a in ((40, 1.0), (40, 0.8), (6, 1.2), (6, 0.9))]
        E0, E1, R0, R1 = [x.astype(np.float64) for x in tabs]
        h, t, r = _facts(rng, 40, 6, 5)
        if cplx:
            qn = np.concatenate([_sq(E0[h] * R0[r] - E1[h] * R1[r]) + _sq(E0[h] * R1[r] + E1[h] * R0[r]),
                                 _sq(R0[r] * E0[t] + R1[r] * E1[t]) + _sq(R0[r] * E1[t] - R1[r] * E0[t])])
        else:
            qn = np.concatenate([_sq(E0[h] * R0[r]), _sq(E0[t] * R0[r])])
        fr = ref.scale_log2_frac(qn)
        if np.all((fr > 0.1) & (fr < 0.9)):
            return tabs, (h, t, r)
    raise AssertionError('no seed found')


@pytest.mark.parametrize('qpw', ['4', '16'])
@pytest.mark.parametrize('d,cplx', [(8, False), (56, False), (40, True)])
def test_dot_query_pipeline_operand_bytes(hip, monkeypatch, qpw, d, cplx):
    """kge_lp_dot_query_pipeline: the planar hi operand with PER-QUERY scales and the guard column built from the row's own
    norm, byte for byte from the kernel's own Q / Q1 and qn (an any-order sum: the scale and the guard are functions of it)."""
    lib = hip.load_library()
    monkeypatch.setenv('KGE_DQPIPE_QPW', qpw)
    (E0, E1, R0, R1), (h, t, r) = _dot_queries(d, cplx)
    if not cplx:
        E1 = R1 = None
    K = 2 * d if cplx else d
    em0 = _dev(np.array([_sq(E0).max()], F))
    em1 = _dev(np.array([_sq(E1).max()], F)) if cplx else None
    de2, qmax, ovf = torch.full((1,), 1e-7, device='cuda'), torch.zeros(1, device='cuda'), torch.zeros(1, device='cuda')
    out = hip.lp_dot_query_pipeline(hip.SIDE_BOTH, _dev(E0), _dev(E1), _dev(R0), _dev(R1), _dev(h), _dev(t), _dev(r), em0, em1,
                                    de2, qmax, ovf)
    torch.cuda.synchronize()
    Q0, qn = out['Q'].cpu().numpy(), out['qn'].cpu().numpy()
    Q1 = out['Q1'].cpu().numpy() if cplx else None
    assert ref.scale_is_safe(qn)
    s_q = ref.split_scale(qn)
    Bp, units_p = int(lib.kge_lp_split_rows_padded(10, 1)), int(lib.kge_lp_hi_units(K))
    hi = ref.hi_values(Q0, Q1, Bp, units_p, 3, aug=qn, aug_mul=1.0, scale=s_q, nmax=qn)
    assert np.array_equal(_bytes(out['Qs']), ref.planar_bytes(hi)), (qpw, d, cplx)
    _assert_bound(qn, _sq(Q0) + (_sq(Q1) if cplx else 0.0), 'qn')
    _assert_bound(out['q_dn2'].cpu().numpy(), ref.residuals(Q0, Q1, s_q), 'q_dn2')
    assert float(ovf[0]) == 0.0


@pytest.mark.parametrize('kind,de,dr', [('transh', 64, 64), ('transh', 260, 260), ('transd', 72, 48)])
def test_prep_hi_operand_bytes(hip, kind, de, dr):
    """kge_lp_prep_hi (TransH: all loads in flight at d = 64, the loops at 260; TransD): the planar hi operand of the query
    rows on the fixed scale, two augmentation columns 1, 1, zero rows behind the batch -- from the kernel's own Q0."""
    lib = hip.load_library()
    rng = np.random.default_rng(de + dr)
    E, R = _rows(de, 30, de, 1.0), _rows(de + 1, 6, dr, 0.5)
    if kind == 'transh':
        tables, code = [E, R, _rows(de + 2, 6, dr, 1.0)], hip.TRANSH
    else:
        tables, code = [E, R, _rows(de + 2, 30, de, 0.7), _rows(de + 3, 6, dr, 0.7)], hip.TRANSD
    h, t, r = _facts(rng, 30, 6, 5)
    Q0, _, _, _, Qh, dn2 = hip.lp_prep(code, hip.SIDE_BOTH, [_dev(x) for x in tables], de, dr, _dev(h), _dev(t), _dev(r),
                                       want_hi=True)
    torch.cuda.synchronize()
    Q = Q0.cpu().numpy()
    Bp, units_p = int(lib.kge_lp_split_rows_padded(10, 1)), int(lib.kge_lp_hi_units(dr))
    hi = ref.hi_values(Q, None, Bp, units_p, 2, aug_mul=1.0)
    assert np.array_equal(_bytes(Qh), ref.planar_bytes(hi)), (kind, de, dr)
    _assert_bound(dn2.cpu().numpy(), ref.residuals(Q, None), 'q_dn2')
