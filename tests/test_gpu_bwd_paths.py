"""GPU tests of the host side of every backward (run with -m gpu on an MI355X): which entry points of the library a
backward calls and in which order, the column chunking of gradient rows wider than one kge_segment_sum_* call takes, and
the counting sort kge_key_hist / kge_key_scatter, which no wrapper calls.

1. Launch sequence.  The entry points of libkge_hip.so are wrapped by a recorder (a Python callable assigned to the
   attribute of the CDLL instance) and one backward of every kind -- the 13 codes of _hip.py, ANALOGY, ConvKB -- is run at
   B = 0, 300 (below BWD_SORTED_MIN_BATCH) and 2048 (at it), with the deterministic mode off and on, with every gradient
   needed and with only the relation tables' needed.  The recorded names must equal SEQUENCES, a literal table.
2. Wide rows.  ANALOGY with d_sc = 512, d_c = 300: packed rows of K = 1112 > 1024 columns, two column chunks.
3. Counting sort.  perm is a permutation, keys[perm] ascends, hist is the bincount; the order inside a run is open."""
import contextlib

import pytest
import torch

from tests import analogy_ref as ar
from tests.test_gpu_deterministic import skewed_triples
from tests.test_gpu_layout_contract import TRIPLE_KINDS, GRAD_TOL
from tests.helpers import raw

pytestmark = pytest.mark.gpu

N_ENT, N_REL, D = 40, 5, 8
D_E, D_R = 12, 8                    # TransD, TransR
CONVKB_D, CONVKB_F = 1, 1           # the smallest (emb_dim, n_filters) _hip_convkb.check_dims accepts
KINDS = TRIPLE_KINDS + ['analogy', 'convkb']
BATCHES = (0, 300, 2048)
ENT_TABLES = {'complex': (0, 1), 'transd': (0, 2), 'analogy': (0, 1, 2)}        # the tables h and t index (default: 0)
REL_TABLES = {'convkb': (1,)}       # the tables r indexes (default: every other one; ConvKB's other four are layers)


@pytest.fixture(scope='module')
def libs():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip, _hip_det, _hip_analogy, _hip_convkb
    for m in (_hip, _hip_det, _hip_analogy, _hip_convkb):
        m.load_library()
    return _hip, _hip_det, _hip_analogy, _hip_convkb


# ---------------------------------------------------------------------------
# 1. launch sequence
# ---------------------------------------------------------------------------
def address(a):
    return getattr(a, 'value', a) or 0


@contextlib.contextmanager
def recording(lib, names):
    """Every entry point of ``names`` wrapped on the CDLL instance; yields the list of (name, args) it fills."""
    calls = []
    saved = {name: getattr(lib, name) for name in names}

    def wrap(name, fn):
        def call(*args):
            calls.append((name, args))
            return fn(*args)
        return call
    try:
        for name, fn in saved.items():
            setattr(lib, name, wrap(name, fn))
        yield calls
    finally:
        for name, fn in saved.items():     # the bound function objects themselves: their argtypes stay
            setattr(lib, name, fn)


def entry_points(libs):
    return sorted(set().union(*[m._SIGNATURES for m in libs]))


def n_tables(kind):
    return {'transh': 3, 'complex': 4, 'transd': 4, 'transr': 3, 'analogy': 6, 'convkb': 6}.get(kind, 2)


def needs_of(kind, which):
    nt = n_tables(kind)
    if which == 'all':
        return (True,) * nt
    ent = ENT_TABLES.get(kind, (0,))
    return tuple(i in REL_TABLES.get(kind, [j for j in range(nt) if j not in ent]) for i in range(nt))


def backward_of(libs, kind, B, g):
    """(run, h, r): ``run(needs)`` is one backward of ``kind`` on B triples of tiny tables; h, r: the id tensors it passes."""
    hip, _, A, K = libs

    def T(n, k):
        return (torch.randn(n, k, generator=g) * 0.5).cuda()
    h, t, r = (torch.randint(0, n, (B,), generator=g).cuda() for n in (N_ENT, N_ENT, N_REL))
    go = torch.randn(B, generator=g).cuda()
    if kind == 'analogy':
        ent, rel = [T(N_ENT, k) for k in (4, 2, 2)], [T(N_REL, k) for k in (4, 2, 2)]
        return (lambda needs: A.score_triples_bwd(ent, rel, h, t, r, go, needs)), h, r
    if kind == 'convkb':
        d, F = CONVKB_D, CONVKB_F
        E, R, w, cb, L, lb = T(N_ENT, d), T(N_REL, d), T(F, 3).view(F, 3, 1), T(1, F).view(F), T(2, F * d), T(1, 2).view(2)
        ws = K.prepare(w, cb, L, lb, d)
        s = K.score_triples(E, R, ws, d, F, h, t, r)
        return (lambda needs: K.score_triples_bwd(E, R, ws, d, F, h, t, r, s, go, needs)), h, r
    de, dr = {'transd': (D_E, D_R), 'transr': (D_E, D_R), 'rescal': (D, D * D)}.get(kind, (D, D))
    shapes = {'transh': [(N_ENT, de), (N_REL, de), (N_REL, de)],
              'complex': [(N_ENT, de), (N_ENT, de), (N_REL, de), (N_REL, de)],
              'transd': [(N_ENT, de), (N_REL, dr), (N_ENT, de), (N_REL, dr)],
              'rescal': [(N_ENT, de), (N_REL, de * de)],
              'transr': [(N_ENT, de), (N_REL, dr), (N_REL, dr * de)]}.get(kind, [(N_ENT, de), (N_REL, de)])
    tabs = [T(*s) for s in shapes]
    code = TRIPLE_KINDS.index(kind)
    return (lambda needs: hip.score_triples_bwd(code, tabs, de, dr, h, t, r, go, needs)), h, r


def record_backward(libs, kind, B, det, which):
    """The (name, args) calls of one backward, or the exception it raised."""
    import torchkge_amd as tk
    run, h, r = backward_of(libs, kind, B, torch.Generator().manual_seed(17))
    needs = needs_of(kind, which)
    with tk.deterministic(det):
        with recording(libs[0].load_library(), entry_points(libs)) as calls:
            grads = run(needs)
    torch.cuda.synchronize()
    assert len(grads) == len(needs)
    for g_, n in zip(grads, needs):
        assert (g_ is not None) == n
        if n and B == 0:
            assert not bool(g_.any())
    return calls, h, r


ENTRY = {'analogy': 'kge_analogy_score_triples_bwd', 'convkb': 'kge_convkb_score_triples_bwd'}    # default: kge_score_triples_bwd
TOKENS = {'kge_score_triples_bwd': 'bwd', 'kge_analogy_score_triples_bwd': 'bwd', 'kge_convkb_score_triples_bwd': 'bwd',
          'kge_key_sort': 'sort', 'kge_segment_sum_rows': 'sum', 'kge_segment_sum_ordered': 'sum'}


def short(calls):
    """The recorded names in the words of SEQUENCES: 'bwd' the kind's backward kernel entry, 'sort' kge_key_sort, 'sum'
    kge_segment_sum_rows / kge_segment_sum_ordered (which of the two: asserted from the mode), others without 'kge_'."""
    return ' '.join(TOKENS.get(name, name[4:]) for name, _ in calls)


# {kinds: {needs: {B: (sequence with the deterministic mode off, with it on)}}}.  SEQUENCES_NOTE says where it comes from.
SEQUENCES = {
    'transe_l1 transe_l2 distmult hole': {
        'all': {0: ('bwd', 'bwd'), 300: ('bwd', 'bwd sort sum sort sum'), 2048: ('bwd sort sum sort sum',) * 2},
        'rel': {0: ('bwd', 'bwd'), 300: ('bwd', 'bwd sort sum'), 2048: ('bwd sort sum',) * 2},
    },
    'transh': {
        'all': {0: ('bwd', 'bwd'), 300: ('bwd', 'bwd sort sum sort sum sum'), 2048: ('bwd sort sum sort sum sum',) * 2},
        'rel': {0: ('bwd', 'bwd'), 300: ('bwd', 'bwd sort sum sum'), 2048: ('bwd sort sum sum',) * 2},
    },
    'transd complex': {
        'all': {0: ('bwd', 'bwd'), 300: ('bwd', 'bwd sort sum sum sort sum sum'), 2048: ('bwd sort sum sum sort sum sum',) * 2},
        'rel': {0: ('bwd', 'bwd'), 300: ('bwd', 'bwd sort sum sum'), 2048: ('bwd sort sum sum',) * 2},
    },
    'rescal': {
        'all': {0: ('bwd sum rescal_rel_grad',) * 2, 300: ('bwd sort sum sort rescal_rel_grad',) * 2,
                2048: ('bwd sort sum sort rescal_rel_grad',) * 2},
        'rel': {0: ('bwd rescal_rel_grad',) * 2, 300: ('bwd sort rescal_rel_grad',) * 2, 2048: ('bwd sort rescal_rel_grad',) * 2},
    },
    'toruse_l1 toruse_tl1 toruse_tl2 toruse_tel2': {
        'all': {0: ('bwd sum sum',) * 2, 300: ('bwd sort sum sort sum',) * 2, 2048: ('bwd sort sum sort sum',) * 2},
        'rel': {0: ('bwd sum',) * 2, 300: ('bwd sort sum',) * 2, 2048: ('bwd sort sum',) * 2},
    },
    'transr': {
        'all': {0: ('bwd sum sum transr_rel_grad',) * 2, 300: ('bwd sort sum sort sum transr_rel_grad',) * 2,
                2048: ('bwd sort sum sort sum transr_rel_grad',) * 2},
        'rel': {0: ('bwd sum transr_rel_grad',) * 2, 300: ('bwd sort sum transr_rel_grad',) * 2,
                2048: ('bwd sort sum transr_rel_grad',) * 2},
    },
    'analogy convkb': {
        'all': {0: ('bwd', 'bwd'), 300: ('bwd sort sum sort sum',) * 2, 2048: ('bwd sort sum sort sum',) * 2},
        'rel': {0: ('bwd', 'bwd'), 300: ('bwd sort sum',) * 2, 2048: ('bwd sort sum',) * 2},
    },
}
SEQUENCES_NOTE = """Recorded on an MI355X with this file's recorder (record_backward) at the commit BEFORE the five copies of the
reduction tail became _hip_det.reduce_rows, not from the code under test.  One place is not that recording: the four TorusE
kinds at B = 0.  There the old inline sort called kge_key_sort with n = 0 and the data pointer of an empty tensor (NULL)
as perm; the library refused it (KGE_EINVAL) and the backward raised.  _key_perm does not call the sort for an empty id
list, and the table holds what follows: no sort, and the sums called with n = 0, which return before any launch -- as
RESCAL and TransR were recorded at B = 0."""


def expected(kind, which, B, det):
    for kinds, table in SEQUENCES.items():
        if kind in kinds.split():
            return table[which][B][1 if det else 0]
    raise KeyError(kind)


@pytest.mark.parametrize('kind', KINDS)
def test_launch_sequence_of_every_backward(libs, kind):
    hip = libs[0]
    assert hip.BWD_SORTED_MIN_BATCH == 2048 and sorted(BATCHES) == [0, 300, 2048]
    if kind == 'convkb':
        libs[3].check_dims(CONVKB_D, CONVKB_F)
        for d, F in ((CONVKB_D - 1, CONVKB_F), (CONVKB_D, CONVKB_F - 1)):
            with pytest.raises(RuntimeError):
                libs[3].check_dims(d, F)
    for which in ('all', 'rel'):
        for B in BATCHES:
            for det in (False, True):
                tag = (kind, which, B, det)
                calls, h, r = record_backward(libs, kind, B, det, which)
                print('%s needs %s B = %d det %d: %s' % (kind, which, B, det, short(calls)))
                assert short(calls) == expected(kind, which, B, det), tag
                assert calls[0][0] == ENTRY.get(kind, 'kge_score_triples_bwd'), tag
                sums = {name for name, _ in calls if TOKENS.get(name) == 'sum'}
                assert sums <= {'kge_segment_sum_ordered' if det else 'kge_segment_sum_rows'}, tag
                # one sort per id set at the most, none for an id set none of whose tables is needed
                sorts = [address(args[0]) for name, args in calls if name == 'kge_key_sort']
                ids = {h.data_ptr(): 'ht', r.data_ptr(): 'r'}
                assert all(a in ids for a in sorts), tag
                sets = [ids[a] for a in sorts]
                assert len(set(sets)) == len(sets), tag
                if which == 'rel':
                    assert 'ht' not in sets, tag
                assert [args[1] + args[3] for name, args in calls if name == 'kge_key_sort'] \
                    == [2 * B if s == 'ht' else B for s in sets], tag


# ---------------------------------------------------------------------------
# 2. rows wider than one reduction call
# ---------------------------------------------------------------------------
def test_wide_rows_are_reduced_in_column_chunks(libs):
    """ANALOGY, d_sc = 512, d_c = 300 (K = 1112), B = 64: every table's gradient against the float64 index_add_ of the
    per-triple rows (float64 autograd with the gathered rows as leaves), with the metric of
    tests/test_gpu_triple_kernels.py: m_X = max_i max |G[i, X]| / |go_i|, S_rho = the sum of |go_i| m_X over the triples
    that hit row rho, |got - ref| <= GRAD_TOL S_rho elementwise, rows no triple hits bit-zero."""
    import torchkge_amd as tk
    _, det_mod, A, _ = libs
    d_sc, d_c, B = 512, 300, 64
    K = d_sc + 2 * d_c
    assert K > 1024
    g = torch.Generator().manual_seed(23)
    scale = K ** (-1.0 / 6)         # a score is a sum of K products of three entries: O(1)
    tabs = [torch.randn(n, k, generator=g) * scale for n, k in ((N_ENT, d_sc), (N_ENT, d_c), (N_ENT, d_c),
                                                                 (N_REL, d_sc), (N_REL, d_c), (N_REL, d_c))]
    h, t, r, go = skewed_triples(B, N_ENT - 5, N_REL - 1, g)        # the last 5 entities / last relation: never indexed
    assert bool((go != 0).all())
    ht, ar_ = torch.cat([h, t]), torch.arange(B)
    leaves = [x[ht if X < 3 else r].double().requires_grad_(True) for X, x in enumerate(tabs)]
    (ar.sf64(leaves, ar_, B + ar_, ar_) * go.double()).sum().backward()
    ref, S, hit = [], [], []
    for X, (x, leaf) in enumerate(zip(tabs, leaves)):
        keys = ht if X < 3 else r
        G = leaf.grad
        ago = go.abs().double().repeat(keys.shape[0] // B)
        m = (G.abs().amax(1) / ago).max()
        ref.append(torch.zeros(x.shape, dtype=torch.float64).index_add_(0, keys, G))
        S.append(torch.zeros(x.shape[0], dtype=torch.float64).index_add_(0, keys, ago * m))
        hit.append(torch.zeros(x.shape[0]).index_add_(0, keys, torch.ones(keys.shape[0])) > 0)
        assert not bool(hit[-1].all())
    dev = [x.cuda() for x in tabs]
    dh, dt, dr, dgo = (x.cuda() for x in (h, t, r, go))
    for det in (False, True):
        before = dict(det_mod.CALLS)
        with tk.deterministic(det):
            runs = [A.score_triples_bwd(dev[:3], dev[3:], dh, dt, dr, dgo, (True,) * 6) for _ in range(2)]
        torch.cuda.synchronize()
        # two id sets, two column chunks each, two backwards
        assert det_mod.CALLS['ordered' if det else 'atomic'] - before['ordered' if det else 'atomic'] == 8
        assert det_mod.CALLS['atomic' if det else 'ordered'] == before['atomic' if det else 'ordered']
        for X, got in enumerate(runs[0]):
            got = got.cpu()
            assert got.shape == tabs[X].shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all()), X
            assert not bool(got[~hit[X]].contiguous().view(torch.int32).any()), X
            err = (got.double() - ref[X]).abs().amax(1)
            q = float(torch.where(err == 0, torch.zeros_like(err), err / S[X]).max())
            print('wide rows det %d table %d: max |grad - float64| / S_row = %.3g' % (det, X, q))
            assert q <= GRAD_TOL, (det, X, q)
        if det:
            for a, b in zip(*runs):
                assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# 3. the counting sort
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 5000])
def test_counting_sort_orders_the_keys(libs, n):
    """kge_key_hist, the exclusive cumsum of the histogram, kge_key_scatter on [k0 | k1]: keys < 37, key 5 holds half."""
    lib = libs[0].load_library()
    n_keys = 37
    g = torch.Generator().manual_seed(100 + n)
    keys = torch.randint(0, n_keys, (n,), generator=g)
    keys[torch.randperm(n, generator=g)[:n // 2]] = 5
    for n0 in sorted({n, n // 3}):
        dk = keys.cuda()
        k0, k1 = dk[:n0].contiguous(), (dk[n0:].contiguous() if n0 < n else None)
        cnt = torch.zeros(2, n_keys, dtype=torch.int32, device='cuda')
        perm = torch.full((max(n, 1),), -1, dtype=torch.int64, device='cuda')
        assert raw(lib, 'kge_key_hist', k0 if n0 else None, n0, k1, n - n0, cnt[0]) == 0
        off = torch.cumsum(cnt[0], 0, dtype=torch.int64) - cnt[0]
        assert raw(lib, 'kge_key_scatter', k0 if n0 else None, n0, k1, n - n0, off, cnt[1], perm) == 0
        torch.cuda.synchronize()
        assert torch.equal(cnt[0].cpu().long(), torch.bincount(keys, minlength=n_keys)), (n, n0)
        p = perm[:n].cpu()
        assert torch.equal(torch.sort(p).values, torch.arange(n)), (n, n0)
        assert bool((keys[p][1:] >= keys[p][:-1]).all()), (n, n0)
        if n == 0:
            assert int(perm[0]) == -1
