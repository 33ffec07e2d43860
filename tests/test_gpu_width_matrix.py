"""The count sweeps of the split prefilter at every row-width bucket (tests/width_table.py), on both levels.

Layer A: the kernels through LpProblem -- every form x route at every table width against the CPU fmaf chains of
         oracle/kge_oracle.c (the header's bit contract): integer counts, no tolerance.
Layer B: the fused preparation paths the evaluator uses (table / query pipelines, projection query statistics) through
         Model.lp_problem, split counts against the exact fp32 counts.
Layer C: LinkPredictionEvaluator at the widths where the one-product route changes: no setting raises, every setting
         leaves the same ranks, the exact path's ranks lie inside the float64 tie intervals of the oracle.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests import width_table as wt
from tests.helpers import oracle_clib, fptr
from tests.operand_ref import planar_halves
from tests.test_gpu_parity import build_model
from torchkge_amd import _hip as _hip_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    _hip_host.load_library()
    return _hip_host



# the table asserts its own buckets when this module is collected (no GPU needed for that)
wt.verify(_hip_host)

i64 = ctypes.c_int64
B_Q = 200           # two query panels at 96, 128 or 192 queries, the last one partial
N_REL = 7
PLAIN, PROJ = ('l2', 'l2q', 'dot', 'dot2'), ('projh', 'projd')
LONG = 1022         # from here on: fewer candidates, true entities placed by rank (the one-product band is ~1 % of the bulk)


def _n_cand(K):
    return 700 if K < LONG else 300         # partial candidate tiles either way; B N K < 3e8 per reference call


def _widths(form):
    # the projection forms take float4-readable rows at the split level: the nearest admissible width on each side of an edge
    if form == 'l2q':       # where the low augmentation column sits in a unit of its own, or opens one
        return [K for K in wt.WIDTHS if K % 16 in (15, 0)]
    return [K for K in wt.WIDTHS if (form in PLAIN or K % 4 == 0) and not (form == 'dot2' and K < 2)]


def _frag_route(form, K):
    """Does kge_lp_split_count take a fragment-major table for this form (the capability functions, not the table)?"""
    return bool(_hip_host.hi_stream_ok(K)) and (form in PLAIN or _hip_host.hi_stream_panel_ok(K))


def _seg0(K):
    """K0 of the two-segment DOT form: uneven, and the K0 | K1 seam inside a k16 unit (and inside an 8-block of the chain)."""
    k0 = max(1, (K * 3) // 7)
    if k0 % 8 == 0:
        k0 += 5
    return min(k0, K - 1)


def _sqn(lib, X):
    out = np.empty(X.shape[0], dtype=np.float32)
    lib.orc_row_sqnorm_chain(fptr(X), i64(X.shape[1]), i64(X.shape[0]), i64(X.shape[1]), fptr(out))
    return out


def _unit(x):
    return torch.nn.functional.normalize(x, dim=1)


def _spread(E, g):
    """Row norms spread over [0.8, 1.2].  Unit rows would hide the LOW augmentation column of the one-product operands: it
    carries -||e||^2 / 2 minus its f16 rounding, and -1/2 is an f16 -- with unit rows a builder or a sweep that loses that
    column changes no count (found by mutation: both stayed green on unit-norm tables)."""
    return E * (0.8 + 0.4 * torch.rand(E.shape[0], 1, generator=g))


def _by_rank(ref, true, keep, g):
    """True entities at chosen ranks of the reference rows (as test_split_one_product_level_long_rows_chunked_panel: most
    where a fitted model's sit, one query in eight at rank 5 %, four in the bulk); queries in `keep` stay as they are."""
    B, N = ref.shape
    rank_of = np.full(B, max(1, N // 500))
    rank_of[::8] = max(1, N // 20)
    rank_of[torch.randperm(B, generator=g)[:4].numpy()] = N // 2
    order = np.argsort(-ref, axis=1, kind='stable')
    out = order[np.arange(B), rank_of]
    out[keep] = true[keep]
    return out


@functools.lru_cache(maxsize=3)
def _case(form, K):
    """Inputs (CPU, packed), the chain reference's counts and the true entities of one form at one width."""
    lib = oracle_clib()
    B, N = B_Q, _n_cand(K)
    g = torch.Generator().manual_seed(1000 * (PLAIN + PROJ).index(form) + K)
    c = {'form': form, 'K': K, 'B': B, 'N': N}
    ref = np.empty((B, N), dtype=np.float32)
    true = torch.randint(0, N, (B,), generator=g).numpy()
    keep = np.zeros(B, dtype=bool)
    if form in ('l2', 'l2q'):
        # entities around unit norm, q = e + a small r.  K = 1: unit rows are +-1 and half the table ties with every true entity
        # (more re-scored pairs than B N / 4 by the data alone), so the single column keeps its magnitude there
        E = _spread(_unit(torch.randn(N, K, generator=g)), g) if K > 1 else torch.randn(N, K, generator=g)
        R = torch.randn(N_REL, K, generator=g) * (0.6 / K ** 0.5)
        if form == 'l2q':
            # every element a multiple of 2^-8, sums included: the f16 operands are EXACT, the one-product band shrinks to
            # its accumulation terms -- and what is left of a count's error budget no longer hides the low augmentation
            # column (-||e||^2 / 2 is no f16).  On rounded operands a lost column stayed inside the band: two mutations
            # stayed green there
            E, R = torch.round(E * 256) / 256, torch.round(R * 256) / 256
        for j, row in enumerate((N // 2, N // 3, N - 1)):       # exact duplicates of three true rows: ties
            true[j] = j
            E[row] = E[j]
        keep[:3] = True
        q = (E[torch.randint(0, N, (B,), generator=g)] + R[torch.randint(0, N_REL, (B,), generator=g)]).contiguous()
        c['E'], c['q'] = E.contiguous(), q
        c['en'], c['qn'] = _sqn(lib, c['E'].numpy()), _sqn(lib, q.numpy())
        lib.orc_lp_gemm_chain(fptr(q.numpy()), i64(K), fptr(c['E'].numpy()), i64(K), i64(K), None, i64(0), None, i64(0), i64(0),
                              i64(B), i64(N), 1, fptr(c['qn']), fptr(c['en']), fptr(ref))
    elif form in ('dot', 'dot2'):
        K0 = K if form == 'dot' else _seg0(K)
        K1 = K - K0
        T, A = torch.randn(N, K, generator=g), torch.randn(B, K, generator=g)
        A[0] = 0.0                                              # an all-zero query: every score ties at 0
        keep[0] = True
        c['T0'], c['A0'] = T[:, :K0].contiguous(), A[:, :K0].contiguous()
        c['T1'], c['A1'] = (T[:, K0:].contiguous(), A[:, K0:].contiguous()) if K1 else (None, None)
        c['K0'], c['K1'] = K0, K1
        lib.orc_lp_gemm_chain(fptr(c['A0'].numpy()), i64(K0), fptr(c['T0'].numpy()), i64(K0), i64(K0),
                              fptr(c['A1'].numpy()) if K1 else None, i64(K1), fptr(c['T1'].numpy()) if K1 else None, i64(K1),
                              i64(K1), i64(B), i64(N), 0, None, None, fptr(ref))
    else:
        T, W = _spread(_unit(torch.randn(N, K, generator=g)), g), _unit(torch.randn(N_REL, K, generator=g))
        r_idx = torch.randint(0, N_REL, (B,), generator=g)
        # two relation-sorted halves, like a both-sides batch (how the evaluator feeds these modes)
        r_idx = torch.cat([r_idx[:B // 2].sort().values, r_idx[B // 2:].sort().values])
        A = (T[torch.randint(0, N, (B,), generator=g)] + 0.7 * _unit(torch.randn(B, K, generator=g))).contiguous()
        Wq = W[r_idx]
        X = (W @ T.t()).contiguous()                            # inputs of both sides: any values would do
        yc = (torch.randn(N, generator=g) * 0.3).contiguous()
        aw, ww = (A * Wq).sum(1), (Wq * Wq).sum(1)
        pz = (torch.stack([2.0 * aw, ww - 2.0], 1) if form == 'projh' else torch.stack([-2.0 * aw, ww], 1)).contiguous()
        c.update({'T': T.contiguous(), 'A': A, 'X': X, 'yc': yc, 'pz': pz, 'r_idx': r_idx.contiguous()})
        c['en'], c['qn'] = _sqn(lib, c['T'].numpy()), _sqn(lib, A.numpy())
        lib.orc_lp_proj_chain(ctypes.c_int(4 if form == 'projh' else 5), fptr(A.numpy()), i64(K), fptr(c['T'].numpy()), i64(K),
                              i64(K), i64(B), i64(N), fptr(c['qn']), fptr(c['en']), fptr(X.numpy()), i64(N),
                              fptr(c['r_idx'].numpy()), fptr(yc.numpy()), fptr(pz.numpy()), fptr(ref))
    if K >= LONG:
        true = _by_rank(ref, true, keep, g)
    c['true'] = torch.from_numpy(np.ascontiguousarray(true)).long()
    c['s_true'] = ref[np.arange(B), true].copy()
    c['want'] = (ref >= c['s_true'][:, None]).sum(1).astype(np.int32)
    return c


def _on_gpu(hip, c):
    """(problem, candidate-table arguments, the scalars every split dict of the form carries, guard vector)."""
    form, N = c['form'], c['N']
    guard = torch.zeros(8, device='cuda')
    if form in ('l2', 'l2q'):
        dE, dq = c['E'].cuda(), c['q'].cuda()
        en = hip.row_sqnorm(dE, max_io=guard[1:2]); qn = hip.row_sqnorm(dq, max_io=guard[0:1])
        assert np.array_equal(en.cpu().numpy(), c['en']) and np.array_equal(qn.cpu().numpy(), c['qn'])
        return hip.LpProblem(hip.LP_L2_EXPAND, dq, dE, qn=qn, en=en), (dE, {'aug': en}), {}, guard
    if form in ('dot', 'dot2'):
        T0, A0 = c['T0'].cuda(), c['A0'].cuda()
        T1, A1 = (c['T1'].cuda(), c['A1'].cuda()) if c['K1'] else (None, None)
        hip.row_sqnorm(T0, max_io=guard[1:2])
        nm1 = None
        if T1 is not None:
            hip.row_sqnorm(T1, max_io=guard[5:6])
            nm1 = guard[5:6]
        return (hip.LpProblem(hip.LP_DOT, A0, T0, A1=A1, T1=T1),
                (T0, {'X1': T1, 'dot': True, 'nmax0': guard[1:2], 'nmax1': nm1}), {'enmax1': nm1}, guard)
    dT, dA = c['T'].cuda(), c['A'].cuda()
    Np = hip.padded_cols(N)
    Xb, ycb = torch.zeros(N_REL, Np, device='cuda'), torch.zeros(Np, device='cuda')
    Xb[:, :N] = c['X'].cuda()
    ycb[:N] = c['yc'].cuda()
    en = hip.row_sqnorm(dT, max_io=guard[1:2]); qn = hip.row_sqnorm(dA, max_io=guard[0:1])
    assert np.array_equal(en.cpu().numpy(), c['en']) and np.array_equal(qn.cpu().numpy(), c['qn'])
    hip.absmax(Xb, guard[3:4]); hip.absmax(ycb, guard[4:5])
    D = form == 'projd'
    prob = hip.LpProblem(hip.LP_L2_PROJD if D else hip.LP_L2_PROJH, dA, dT, qn=qn, en=en, Wq=c['pz'].cuda(), scal=Xb[:, :N],
                         r_idx=c['r_idx'].cuda(), yc=ycb[:N] if D else None)
    return prob, (dT, {'aug': en}), {'xabsmax': guard[3:4], 'yabsmax': guard[4:5] if D else None}, guard


def _split_dict(hip, route, table, extra, guard):
    X, how = table
    sp = {'enmax': guard[1:2], 'overflow': guard[2:3], 'list_stat': guard[6:7]}
    sp.update(extra)
    if route == 'three':
        Es, e2 = hip.split_table(X, **how)
        sp.update({'Es': Es, 'e2pref': e2})
    else:
        Eh, de2 = hip.hi_table(X, frag=route == 'frag', **how)
        sp.update({'Es': Eh, 'e2pref': None, 'level': 1, 'de2max': de2, 'es_frag': route == 'frag'})
    return sp


def _eps_of(route, K):
    # the shrunken bands of the existing tests: 1/16 on three products; 0.5 on one product from K = 200 (its residual
    # term bounds actual f16 roundings by Cauchy-Schwarz: tight at small K)
    return (1.0, 1.0 / 16) if route == 'three' else ((1.0, 0.5) if K >= 200 else (1.0,))


def _run_route(hip, prob, guard, route, K, st, want, tag):
    """Counts of one route == the reference's, and none of the ways to pass by falling back."""
    B, N = prob.B, prob.N
    try:
        for eps in _eps_of(route, K):
            hip.SPLIT_EPS_SCALE = eps
            guard[6] = 0
            got = prob.count_ge(st).cpu().numpy()
            n_unc = int(prob.last_split[0].item())
            print('%s eps %g: %d re-scored pairs, overflow %g, %d counts differ'
                  % (tag, eps, n_unc, float(guard[2]), int((got != want).sum())))
            assert float(guard[2]) == 0.0, (tag, eps, 'list overflow')
            assert np.array_equal(got, want), (tag, eps, int((got != want).sum()))
            assert B <= n_unc < B * N / 4, (tag, eps, n_unc)        # every true entity is re-scored, the bulk is not
            assert float(guard[6]) == n_unc, (tag, eps)             # ... and reported to the level policy
    finally:
        hip.SPLIT_EPS_SCALE = 1.0


def _layer_a_cases():
    out = []
    for form in PLAIN + PROJ:
        for K in _widths(form):
            for route in ('exact', 'three', 'planar', 'frag'):
                if route == 'frag' and not wt.frag_ok(K, proj=form in PROJ):
                    continue
                out.append(pytest.param(form, K, route, id='%s-K%d-%s' % (form, K, route)))
    return out


@pytest.mark.parametrize('form,K,route', _layer_a_cases())
def test_count_routes_equal_the_chain_reference(hip, form, K, route):
    """Layer A.  exact: kge_lp_count_ge (and the pair scores, bit for bit); three: kge_lp_split_rows + the three-product
    sweep; planar / frag: kge_lp_hi_rows(_frag) + the one-product sweep the width table names -- each followed by the exact
    recheck, each equal to #{c: ref[i, c] >= ref[i, true_i]} of the CPU chain."""
    c = _case(form, K)
    prob, table, extra, guard = _on_gpu(hip, c)
    # what the table says of this width is what the capability functions say for this form
    assert _frag_route(form, K) == wt.frag_ok(K, proj=form in PROJ)
    assert int(hip.load_library().kge_lp_split_regions_supported(ctypes.byref(prob.desc))) == \
        int(wt.units1(K) <= wt.PANEL_UNITS and all(k % 4 == 0 for k in (int(prob.desc.K0), int(prob.desc.K1))))
    st = prob.pair_scores(c['true'].cuda())
    assert np.array_equal(st.cpu().numpy(), c['s_true'])
    if route == 'exact':
        assert prob.split is None
        assert np.array_equal(prob.count_ge(st).cpu().numpy(), c['want'])
        assert int(c['want'].min()) >= 1 and (form not in ('dot', 'dot2') or int(c['want'][0]) == c['N'])
        return
    prob.split = _split_dict(hip, route, table, extra, guard)
    _run_route(hip, prob, guard, route, K, st, c['want'], '%s K=%d %s' % (form, K, route))


@pytest.mark.parametrize('K', [13, 14, 15, 16, 17, 205, 206, 207, 510, 511])
def test_one_product_table_carries_both_augmentation_columns(hip, K):
    """kge_lp_hi_rows / kge_lp_hi_rows_frag, L2 candidates: column K holds the f16 of -||e||^2 / 2 (scaled), column K + 1 the
    f16 of what that rounding left -- in the same unit, filling it, or one unit further -- the data columns their f16,
    everything behind zero, padding rows -65504 in both.  (The count tests cannot see the second column on rounded
    operands: it is smaller than the band.)"""
    N = 100
    g = torch.Generator().manual_seed(K)
    E = _spread(_unit(torch.randn(N, K, generator=g)), g)
    dE = E.cuda()
    en = hip.row_sqnorm(dE)
    lib = hip.load_library()
    units_p, rows_p = int(lib.kge_lp_hi_units(K)), int(lib.kge_lp_split_rows_padded(N, 0))
    assert units_p * 16 >= K + 2
    got = [planar_halves(hip.hi_table(dE, aug=en, frag=frag)[0], rows_p, units_p, frag) for frag in (False, True)]
    assert torch.equal(got[0], got[1])
    H = got[0]
    scale = float(2.0 ** torch.round(torch.log2((H[:N, 0] / E[:, 0]).abs().median())))      # the operands' power-of-two scale
    assert torch.equal(H[:N, :K], (E * scale).half().float())
    full = en.cpu() * -0.5 * scale
    hi = full.half().float()
    lo = (full - hi).half().float()
    assert int((lo != 0).sum()) > N // 2
    assert torch.equal(H[:N, K], hi) and torch.equal(H[:N, K + 1], lo)
    assert not bool(H[:N, K + 2:].any())
    assert bool((H[N:, K] == -65504.0).all()) and bool((H[N:, K + 1] == -65504.0).all())


# grouped query columns (ColumnPlan) on the plain forms: the runtime loop, the 13- and 26-unit bodies, both sides of the
# grouped kernel's 4-wave | 8-wave flip (19 | 20 units), one width above 26 units, the longest resident panel, and beyond it
# (chunked / planar only: split_prepare drops the grouped columns on a fragment-major table, the planar kernel keeps them)
@pytest.mark.parametrize('form,K,route', [pytest.param(f, K, rt, id='%s-K%d-%s' % (f, K, rt)) for f in ('l2', 'dot')
                                          for K in (17, 206, 302, 303, 414, 415, 510, 511, 600)
                                          for rt in ('three', 'planar', 'frag') if rt != 'frag' or wt.frag_ok(K)])
def test_count_routes_on_query_columns_equal_the_chain_reference(hip, form, K, route):
    from torchkge_amd.filter_index import ColumnPlan
    lib = oracle_clib()
    N, nb = 700, B_Q // 2
    g = torch.Generator().manual_seed(77 * K + (form == 'dot'))
    h = torch.randint(0, N // 20, (nb,), generator=g); t = torch.randint(0, N, (nb,), generator=g)
    r = torch.randint(0, 3, (nb,), generator=g)
    h[:40], r[:40] = 1, 0                           # one key with 40 queries: ten grouped columns
    true = torch.cat([t, h])
    guard = torch.zeros(8, device='cuda')
    ref = np.empty((2 * nb, N), dtype=np.float32)
    if form == 'l2':
        E = _spread(_unit(torch.randn(N, K, generator=g)), g)
        R = torch.randn(N_REL, K, generator=g) * (0.6 / K ** 0.5)
        q = torch.cat([E[h] + R[r], E[t] - R[r]]).contiguous()
        en_, qn_ = _sqn(lib, E.numpy()), _sqn(lib, q.numpy())
        lib.orc_lp_gemm_chain(fptr(q.numpy()), i64(K), fptr(E.numpy()), i64(K), i64(K), None, i64(0), None, i64(0), i64(0),
                              i64(2 * nb), i64(N), 1, fptr(qn_), fptr(en_), fptr(ref))
        dE, dq = E.cuda(), q.cuda()
        en = hip.row_sqnorm(dE, max_io=guard[1:2]); qn = hip.row_sqnorm(dq, max_io=guard[0:1])
        prob, table, extra = hip.LpProblem(hip.LP_L2_EXPAND, dq, dE, qn=qn, en=en), (dE, {'aug': en}), {}
    else:
        E, R = torch.randn(N, K, generator=g), torch.randn(N_REL, K, generator=g)
        q = torch.cat([E[h] * R[r], E[t] * R[r]]).contiguous()
        lib.orc_lp_gemm_chain(fptr(q.numpy()), i64(K), fptr(E.numpy()), i64(K), i64(K), None, i64(0), None, i64(0), i64(0),
                              i64(2 * nb), i64(N), 0, None, None, fptr(ref))
        dE, dq = E.cuda(), q.cuda()
        hip.row_sqnorm(dE, max_io=guard[1:2])
        prob = hip.LpProblem(hip.LP_DOT, dq, dE)
        table, extra = (dE, {'dot': True, 'nmax0': guard[1:2], 'nmax1': None}), {'enmax1': None}
    s_true = ref[np.arange(2 * nb), true.numpy()]
    want = (ref >= s_true[:, None]).sum(1).astype(np.int32)
    cols = ColumnPlan(h.cuda(), t.cuda(), r.cuda(), N, N_REL, hip.split_group_sets(), hip.split_query_rows_padded)
    assert cols.n_multi > 0 and cols.n_single > 0
    st = prob.pair_scores(true.cuda())
    assert np.array_equal(st.cpu().numpy(), s_true)
    prob.split = _split_dict(hip, route, table, extra, guard)
    prob.cols = cols
    _run_route(hip, prob, guard, route, K, st, want, '%s K=%d %s columns' % (form, K, route))
    if route == 'frag':     # grouped columns stay on the free-running sweep exactly on its resident panel
        assert (prob.cols is not None) == (wt.units1(K) <= wt.PANEL_UNITS)


# ---------------------------------------------------------------------------
# Layer B: the fused preparation paths through the models
# ---------------------------------------------------------------------------
N_ENT, N_RELS = 600, 9
# the model layers want d % 8 == 0 (ComplEx sweeps 2 d columns); 203 / ComplEx d = 100: the general paths
MODEL_WIDTHS = [K for K in wt.WIDTHS if K % 8 == 0 and K <= 1040] + [203, 332]
KINDS = ('transe', 'distmult', 'complex', 'transh', 'transd')


def _model(kind, K, seed=3, spread=False):
    d = K // 2 if kind == 'complex' else K
    tables = orc.init_tables(kind, N_ENT, N_RELS, d, seed=seed, d_rel=d if kind == 'transd' else None)
    if spread and kind in ('transe', 'transh', 'transd'):
        # entities inside the unit ball, as between two normalisations of a training run (see _spread: unit rows hide the
        # low augmentation column kge_lp_table_prep_l2 writes)
        tables[0] = tables[0] * (0.8 + 0.2 * torch.rand(N_ENT, 1, generator=torch.Generator().manual_seed(seed + K)))
    return build_model(kind, 2, tables, N_ENT, N_RELS), tables


def _layer_b_cases():
    out = []
    for kind in KINDS:
        for K in sorted(MODEL_WIDTHS):
            if kind == 'complex' and K % 2:
                continue
            if kind == 'complex' and K % 16 and K != 200:       # (d = 100: its one general-path width)
                continue
            out.append(pytest.param(kind, K, id='%s-K%d' % (kind, K)))
    return out


@pytest.mark.parametrize('kind,K', _layer_b_cases())
def test_model_problems_split_counts_equal_exact_counts(hip, kind, K):
    """Layer B.  What evaluate() runs per batch -- kge_lp_table_prep_l2, kge_lp_dot_table_prep(_fused),
    kge_lp_query_pipeline, kge_lp_dot_query_pipeline, kge_proj_query_stats, each with its own augmentation and tail code --
    through Model.lp_problem('both') inside a guarded session, on both levels: counts == kge_lp_count_ge's, no overflow, and
    the fragment-major table exactly where the width table says this model's mode has a sweep for it."""
    m, _ = _model(kind, K, spread=True)
    assert m._lp_width() == K
    g = torch.Generator().manual_seed(K)
    n = 300
    r = torch.randint(0, N_RELS, (n,), generator=g).sort().values
    h, t = torch.randint(0, N_ENT, (n,), generator=g), torch.randint(0, N_ENT, (n,), generator=g)
    hb, tb, rb = h.cuda(), t.cuda(), r.cuda()
    true = torch.cat([tb, hb])
    proj = kind in ('transh', 'transd')
    # (TransE rows that are not float4-readable leave the fused query pipeline: that path stays on three products)
    levels = {0: 0, 1: 0 if (kind == 'transe' and K % 4) else 1}
    try:
        for forced, level in levels.items():
            m.split_level = forced
            guard = m.lp_guard_begin(torch.device('cuda', 0))
            try:
                guard.zero_()
                with m.lp_session():
                    prob = m.lp_problem(hb, tb, rb, 'both')
                    assert prob.split is not None and int(prob.split.get('level', 0)) == level, (kind, K, level)
                    assert bool(prob.split.get('es_frag')) == (level == 1 and wt.frag_ok(K, proj=proj)), (kind, K, level)
                    if prob.pre is not None:
                        prob.pre['true_idx'] = true
                    st = prob.pair_scores(true)
                    prep = prob.split_prepare()
                    raw = torch.zeros(prob.B, dtype=torch.int32, device='cuda')
                    prob.split_count(prep, st, raw)
                    prob.split_recheck(prep, st, raw)
                    n_unc = int(prep['n_list'].item())
                    prob.split = None
                    prob.cols = None
                    exact = prob.count_ge(st)
                    print('%s K=%d level %d: %d re-scored pairs, overflow %g' % (kind, K, level, n_unc, float(guard[2])))
                    assert float(guard[2]) == 0.0, (kind, K, level, 'overflow')
                    assert torch.equal(raw, exact), (kind, K, level, int((raw != exact).sum()))
                    assert prob.B == 2 * n and n_unc >= prob.B and int(exact.min()) >= 1
            finally:
                m.lp_guard_end()
    finally:
        m.split_level = 'auto'


# ---------------------------------------------------------------------------
# Layer C: the evaluator never raises and never changes a rank
# ---------------------------------------------------------------------------
EVAL_CASES = [(k, K) for k in ('transh', 'transd') for K in (496, 512, 528, 1024, 1040)] + \
             [(k, K) for k in ('transe', 'distmult') for K in (512, 528, 1024)] + \
             [('complex', 2 * d) for d in (256, 264, 512, 1016, 1024)]


@functools.lru_cache(maxsize=1)
def _graph():
    import torchkge_amd as tk
    h, t, r = orc.synthetic_triples_zipf(N_ENT, N_RELS, 3000, 41, hubs=((150, 'head'), (60, 'tail')))
    kg = tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(N_ENT)},
                           rel2ix={i: i for i in range(N_RELS)})
    _, kg_test = kg.split_kg(sizes=(2700, 300))
    dh, dt, _ = orc.build_filter_dicts(h, t, r)
    return kg_test, dh, dt


def _ranks(ev):
    return [ev.rank_true_heads.clone(), ev.rank_true_tails.clone(), ev.filt_rank_true_heads.clone(),
            ev.filt_rank_true_tails.clone()]


@pytest.mark.parametrize('kind,K', [pytest.param(k, K, id='%s-K%d' % (k, K)) for k, K in EVAL_CASES])
def test_evaluator_every_setting_same_ranks(hip, kind, K):
    """Layer C.  split_filter off (the exact path), split_level 0, split_level 1 eager and as hipGraph replays, and the
    'auto' policy entering and leaving level 1: no setting raises (TransH / TransD at 33 / 65 units raised
    'kge_lp_split_count rejected its arguments (code -3)' from level 1; ComplEx d = 1024 has no prefix maxima), all four
    rank vectors identical, the exact path's inside the oracle's float64 tie intervals."""
    import torchkge_amd as tk
    import torchkge_amd.evaluation as evm
    assert K in wt.ROW
    kg_test, dh, dt = _graph()
    m, tables = _model(kind, K, seed=5)
    proj = kind in ('transh', 'transd')
    # which one-product route this model is on: the capability functions and the table agree
    want_frag = _hip_host.hi_stream_ok(K) and (not proj or _hip_host.hi_stream_panel_ok(K))
    assert m._level1_stream() == bool(want_frag)
    assert bool(want_frag) == wt.frag_ok(K, proj=proj)
    try:
        m.split_filter = False
        ev = tk.LinkPredictionEvaluator(m, kg_test, graph=False)
        ev.evaluate(128, verbose=False)
        want = _ranks(ev)
        m.split_filter = True
        scale = float(tables[0].pow(2).sum(1).max()) * 4 + 1.0
        ties = orc.lp_evaluate(kind, [x.double() for x in tables], kg_test.head_idx, kg_test.tail_idx, kg_test.relations,
                               dh, dt, 32, 2, tie_tol=4e-6 * scale)[4]
        for k in range(4):
            assert bool(((want[k].cpu() >= ties[k, :, 0]) & (want[k].cpu() <= ties[k, :, 1])).all()), (kind, K, k)
        m.split_level = 0
        ev0 = tk.LinkPredictionEvaluator(m, kg_test, graph=False)
        ev0.evaluate(128, verbose=False)
        assert ev0._level == 0
        for a, b in zip(want, _ranks(ev0)):
            assert torch.equal(a, b), (kind, K, 'level 0')
        m.split_level = 1
        for graph in (False, True):
            ev1 = tk.LinkPredictionEvaluator(m, kg_test, graph=graph)
            ev1._level = 1
            for _ in range(3):
                ev1.evaluate(128, verbose=False)
                for a, b in zip(want, _ranks(ev1)):
                    assert torch.equal(a, b), (kind, K, 'level 1', graph)
        m.split_level = 'auto'
        old = evm.LEVEL1_ENTER, evm.LEVEL1_LEAVE
        try:
            evm.LEVEL1_ENTER, evm.LEVEL1_LEAVE = 1e9, 1e9        # always enter, never leave
            ev2 = tk.LinkPredictionEvaluator(m, kg_test)
            seen = []
            for _ in range(3):
                ev2.evaluate(128, verbose=False)
                seen.append(ev2._level)
                for a, b in zip(want, _ranks(ev2)):
                    assert torch.equal(a, b), (kind, K, 'auto', seen)
            assert seen == [1, 1, 1], seen                       # (the level the NEXT evaluation will use: level 1 ran twice)
            assert not getattr(ev2, '_last_redo', False)         # ... on the one-product sweep itself, not on a redo
            evm.LEVEL1_LEAVE = 0.0                               # ... and leave again at once
            ev2.evaluate(128, verbose=False)
            assert ev2._level == 0
            ev2.evaluate(128, verbose=False)
            for a, b in zip(want, _ranks(ev2)):
                assert torch.equal(a, b), (kind, K, 'auto, left')
        finally:
            evm.LEVEL1_ENTER, evm.LEVEL1_LEAVE = old
    finally:
        m.split_filter = True
        m.split_level = 'auto'
