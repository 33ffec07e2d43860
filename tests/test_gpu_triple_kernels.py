"""GPU tests of the fused triple kernels of torchkge_amd/csrc/score_triples.hip (run with -m gpu on an MI355X):
kge_score_triples, kge_score_triples_bwd (atomic mode and row mode) and, of segment_sum_rows.hip, the
kge_segment_sum_rows that reduces their gradient rows, for the ten kinds they serve -- TransE-L1 / L2, TransH, TransD, DistMult, ComplEx and the four TorusE kinds -- in every row-width bucket
(NE = 4 / 8 / 16 registers per lane, float4 and scalar row loads, the non-pipelined forward of NE = 16), past the grid
cap (the grid-stride loops, the forward's two-set pipeline, segment_sum_kernel's second chunk) and at the edges the code
handles (clamped norms, exact zeros, go == 0 in row mode, h == t, d > 1024 refused).

Reference: float64 autograd of oracle.kge_oracle.score_triples (classic kinds) / of the TorusE restatement with x
substituted by the fp32 value the kernel forms (tests/test_gpu_toruse.py), with the GATHERED rows as leaves, so that
G[i, X] -- triple i's gradient row for table X -- exists on its own and the table gradient is their index_add_.

Metric (gradients): per table X, m_X = max over triples (go_i != 0, no clamped row) of max |G[i, X]| / |go_i|; a triple's
scale is |go_i| m_X, or max |G[i, X]| where the stream's own row is all-zero (its gradient is g / 1e-12: no cancellation);
S_rho = the sum of the scales of the triples that hit row rho; |got - ref| <= GRAD_TOL S_rho elementwise, rows no triple
hits are bit-zero.  One hub row therefore cannot set the bound of the singleton rows.  The same ratio max |x - ref| / S_rho
of the fp32 ATen restatement must stay below GRAD_TOL / 10 (a check on the inputs); both ratios are printed per
(kind, d, mode) -- DESIGN.md section 6 records the largest.

Scores: |s - s64| <= TOL max(1, |s64|), the form in which the suite applies TOL = 1e-5 to these entry points
(close() of tests/test_gpu_layout_contract.py and tests/test_gpu_toruse.py).  A plain |s - s64| <= TOL needs scores of
O(1), and the prescribed inputs do not give them everywhere: a TransE-L1 score is the 1-norm of a difference of unit
vectors, O(sqrt(d)) (44 at d = 1024); a TorusE score is a sum of d terms of O(1); and at d <= 8 the squared-L2 scores
reach (|h^| + |r| + |t^|)^2 = 9..16, where one ulp is 1e-6 and the fp32 ATen restatement itself is 2.7e-6 .. 3.3e-6 off
(measured on the CPU: TransE-L2 d = 1 and d = 8, TransD d = 5 and d = 8).  For d >= 64 the squared-L2, DistMult and
ComplEx scores are <= 4 or so and the two forms differ by that factor at most.  The fp32 restatement must be within a
quarter of the bound: if that fails, the inputs are wrong, not the kernel.  Measured on the MI355X: the kernel's largest
|s - s64| is 0.06 of this bound for the classic kinds and 0.13 for the TorusE kinds.

A normalised row of width 1 is +-1 whatever its value, so its gradient is identically zero (every table of the
normalising kinds at d = 1, R and Rp of TransD at d_rel = 1).  float64 autograd returns its own rounding noise there
(1e-17) and m_X would be that noise; the reference for such a table is therefore exact zero, the kernel must return exact
zeros (x / sqrt(x x) is exactly +-1 in IEEE arithmetic, and g - x^ (x^ . g) exactly 0), and the restatement's noise is
not measured.

TransE-L1: sign(diff) may differ between fp32 and float64 where |diff| is tiny; go_i is set to 0 for every triple with an
element |diff_k| < 1e-5 / sqrt(d) of the float64 normalised diff, computed BEFORE the kernel runs.  (1e-5 in units of
the typical element 1 / sqrt(d) of a normalised row: fp32 rounding of such a diff is ~3e-7 in the same units.  A fixed
1e-5 would zero a share of the batch growing as d^1.5 -- 15 % at d = 1024 -- where this one stays below 0.5 %; at most 3 %
of the batch may be zeroed, which the test asserts.)"""
import math
import os

import pytest
import torch
from torch.nn.functional import normalize

from tests.helpers import raw, carve
from tests.test_gpu_deterministic import skewed_triples, key_cases, nan_padded, U
from tests.test_gpu_layout_contract import TRIPLE_KINDS, TORUS_DISS, N_STREAMS, GRAD_TOL, TOL, triple_tables, triple_sf64
from tests.test_gpu_toruse import diss64

pytestmark = pytest.mark.gpu

KINDS = ['transe_l1', 'transe_l2', 'transh', 'transd', 'distmult', 'complex', 'toruse_l1', 'toruse_tl1', 'toruse_tl2',
         'toruse_tel2']
CODE = {k: TRIPLE_KINDS.index(k) for k in KINDS}                # the KGE_* kind code of the header
ENT = {'complex': (0, 1), 'transd': (0, 2)}                     # the tables indexed by h and t (default: table 0)
NORMALISED = {'transe_l1': (0,), 'transe_l2': (0,), 'distmult': (0,), 'transh': (0, 2), 'transd': (0, 1, 2, 3)}
BWD_KINDS = ['transe_l2', 'transh', 'complex', 'transd']        # one kind per row-set size (3, 4, 6 and 6 with d_rel)
GRID_CAP_BWD_KINDS = BWD_KINDS + ['toruse_tl2']                 # ... and the family without normalisation (row mode only)
DEVICE = 'cuda'
SENTINEL = 0x7FC0BEEF                                           # a quiet NaN with a payload


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


def bits(x):
    return x.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------
# inputs, reference and metric
# ---------------------------------------------------------------------------
def make_tables(kind, de, dr, g, n_ent, n_rel):
    """fp32 tables (CPU) for which scores stay O(1): entity rows randn * 0.5 (norms != 1: the normalisation has work to
    do), translation rows randn / sqrt(d), DistMult relation rows randn * 0.5, ComplEx randn * 0.7 d^-1/4, TorusE rows as
    in triple_tables."""
    def T(n, k, s=0.5):
        return torch.randn(n, k, generator=g) * s
    if kind in TORUS_DISS:
        return triple_tables(kind, de, g, n_ent, n_rel)[0]
    if kind == 'transd':
        return [T(n_ent, de), T(n_rel, dr, 1 / math.sqrt(dr)), T(n_ent, de), T(n_rel, dr)]
    if kind == 'transh':
        return [T(n_ent, de), T(n_rel, de, 1 / math.sqrt(de)), T(n_rel, de)]
    if kind == 'complex':
        return [T(n, de, 0.7 * de ** -0.25) for n in (n_ent, n_ent, n_rel, n_rel)]
    if kind == 'distmult':
        return [T(n_ent, de), T(n_rel, de)]
    return [T(n_ent, de), T(n_rel, de, 1 / math.sqrt(de))]


def make_triples(B, n_ent, n_rel, g):
    """skewed_triples (three quarters of the batch on one head and one relation) with a few h == t, the hub included."""
    h, t, r, go = skewed_triples(B, n_ent, n_rel, g)
    t[0] = h[0]
    t[B - 7:B - 3] = h[B - 7:B - 3]
    return h, t, r, go


def keys_of(kind, X, h, t, r):
    return torch.cat([h, t]) if X in ENT.get(kind, (0,)) else r


def reference(kind, tabs, de, dr, h, t, r, go, dtype):
    """(scores, [G_X]) of the restatement in `dtype` under autograd with the gathered rows as leaves: G_X is (2B, d)
    for an entity table (rows of h, then of t) and (B, d) for a relation table."""
    B = h.shape[0]
    ar = torch.arange(B, device=h.device)
    leaves = [x[keys_of(kind, X, h, t, r)].to(dtype).requires_grad_(True) for X, x in enumerate(tabs)]
    if kind in TORUS_DISS:
        fh, ft, fr = (x - x.detach().trunc() for x in (leaves[0][:B], leaves[0][B:], leaves[1]))
        x = (fh + fr) - ft
        if dtype == torch.float64:      # x as the kernel forms it (frac is exact in fp32): the branches are taken on it
            xf = (fh.detach().float() + fr.detach().float()) - ft.detach().float()
            x = x + (xf.double() - x).detach()
        s = -diss64(TORUS_DISS[kind], x)
    else:
        s = triple_sf64(kind, leaves, de, dr, ar, B + ar, ar)
    (s * go.to(dtype)).sum().backward()
    return s.detach(), [x.grad for x in leaves]


def l1_kinks(tabs, h, t, r, de):
    """Triples of TransE-L1 with an element of the float64 normalised diff inside the band where fp32 may see another
    sign (a diff that is zero in every element has no sign on either side and stays)."""
    E, R = tabs[0].double(), tabs[1].double()
    diff = (normalize(E[h], p=2, dim=1) + R[r]) - normalize(E[t], p=2, dim=1)
    return (diff.abs() < 1e-5 / math.sqrt(de)).any(1) & (diff != 0).any(1)


def row_sum(n, keys, vals):
    """zeros(n, ...).index_add_(0, keys, vals) in vals' dtype.  Summed on the host: three quarters of `keys` are one row,
    and float64 adds to one address from a whole batch at once take seconds on the GPU at the grid-cap batch."""
    out = torch.zeros((n,) + tuple(vals.shape[1:]), dtype=vals.dtype)
    return out.index_add_(0, keys.cpu(), vals.cpu()).to(vals.device)


def score_bound(s64):
    return TOL * s64.abs().clamp_min(1.0)


class Case(object):
    """One (kind, tables, triples, go): the float64 reference, the per-row bounds S_rho and the fp32 restatement, computed
    once and shared by the forward and every backward mode."""

    def __init__(self, kind, tabs, de, dr, h, t, r, go, tag):
        self.kind, self.tabs, self.de, self.dr, self.tag = kind, tabs, de, dr, tag
        self.h, self.t, self.r = h, t, r
        if kind == 'transe_l1':
            kink = l1_kinks(tabs, h, t, r, de)
            share = float(kink.float().mean())
            assert share <= 0.03, (tag, 'share of the batch inside the L1 kink band', share)
            go = torch.where(kink, torch.zeros_like(go), go)
        self.go = go
        self.s64, G64 = reference(kind, tabs, de, dr, h, t, r, go, torch.float64)
        s32, G32 = reference(kind, tabs, de, dr, h, t, r, go, torch.float32)
        self.s_tol = score_bound(self.s64)
        err32 = (s32.double() - self.s64).abs()
        assert bool((err32 <= self.s_tol / 4).all()), (tag, 'fp32 restatement of the scores: the inputs are wrong', float(err32.max()))
        # per-row bounds
        B = h.shape[0]
        normd = NORMALISED.get(kind, ())
        zero = {X: (tabs[X] == 0).all(1) for X in normd}
        uses = torch.zeros(B, dtype=torch.bool, device=h.device)
        for X in normd:
            z = zero[X][keys_of(kind, X, h, t, r)]
            uses |= (z[:B] | z[B:]) if z.shape[0] == 2 * B else z
        ok = (go != 0) & ~uses
        self.rows = []
        self.ratio32 = []
        for X, tab in enumerate(tabs):
            keys = keys_of(kind, X, h, t, r)
            rep = keys.shape[0] // B
            unit = X in normd and tab.shape[1] == 1     # rows of width 1 normalise to +-1: the gradient is exactly zero
            if unit:
                G64[X] = torch.zeros_like(G64[X])
            gmax = G64[X].abs().amax(1)
            ago, okx = go.abs().double().repeat(rep), ok.repeat(rep)
            m = (gmax[okx] / ago[okx]).max() if bool(okx.any()) else gmax.new_zeros(())
            scale = ago * m
            if X in normd:
                scale = torch.where(zero[X][keys], gmax, scale)
            n, d = tab.shape
            self.rows.append((row_sum(n, keys, G64[X]), row_sum(n, keys, scale), row_sum(n, keys, torch.ones_like(scale)) > 0))
            g32 = row_sum(n, keys, G32[X])
            self.ratio32.append(0.0 if unit else self.ratio(X, g32))
        worst = max(self.ratio32)
        assert worst < GRAD_TOL / 10, (tag, 'fp32 restatement of the gradients: the inputs are wrong', self.ratio32)

    def ratio(self, X, got):
        """max |got - ref| / S_rho over table X (0 / 0 = 0, x / 0 = inf); rows no triple hits must be bit-zero."""
        ref, S, hit = self.rows[X]
        assert got.shape == ref.shape and got.dtype == torch.float32, (self.tag, X)
        assert bool(torch.isfinite(got).all()), (self.tag, 'table', X, 'not finite')
        assert not bool(bits(got[~hit]).any()), (self.tag, 'table', X, 'a row that no triple hits is not bit-zero')
        err = (got.double() - ref).abs().amax(1)
        q = torch.where(err == 0, torch.zeros_like(err), err / S)
        return float(q.max())

    def check_scores(self, s):
        assert s.shape == self.s64.shape and bool(torch.isfinite(s).all()), self.tag
        err = (s.double() - self.s64).abs()
        worst = int((err - self.s_tol).argmax())
        print('triple kernels %s scores: max |s - float64| / bound %.3g' % (self.tag, float((err / self.s_tol).max())))
        assert bool((err <= self.s_tol).all()), (self.tag, 'triple', worst, float(err[worst]), float(self.s_tol[worst]))

    def check_grads(self, grads, mode):
        ratios = [self.ratio(X, g) for X, g in enumerate(grads)]
        print('triple kernels %s %s: max |grad - float64| / S_row per table: kernel %s, fp32 restatement %s'
              % (self.tag, mode, ' '.join('%.3g' % q for q in ratios), ' '.join('%.3g' % q for q in self.ratio32)))
        for X, q in enumerate(ratios):
            assert q <= GRAD_TOL, (self.tag, mode, 'table', X, q)
        return ratios


def make_case(kind, de, dr, B, n_ent, n_rel, seed, tag, device=None, off=0, edit=None):
    device = device or DEVICE
    g = torch.Generator().manual_seed(seed)
    tabs = make_tables(kind, de, dr, g, n_ent, n_rel)
    h, t, r, go = make_triples(B, n_ent, n_rel, g)
    if edit is not None:
        edit(tabs, h, t, r, go)
    if off:     # every table `off` floats past a 16-byte boundary (still contiguous): tables_vec4 must say no
        tabs = [carve(x, 0, off, device=device) for x in tabs]
        assert all(x.is_contiguous() and x.data_ptr() % 16 == 4 * off for x in tabs)
    else:
        tabs = [x.to(device) for x in tabs]
    h, t, r, go = (x.to(device) for x in (h, t, r, go))
    return Case(kind, tabs, de, dr, h, t, r, go, tag)


def wrapper_bwd(hip, monkeypatch, case, mode):
    """_hip.score_triples_bwd with the mode forced through BWD_SORTED_MIN_BATCH; the reduction counter tells which ran."""
    from torchkge_amd import _hip_det
    monkeypatch.setattr(hip, 'BWD_SORTED_MIN_BATCH', 0 if mode == 'rows' else 1 << 62)
    nt = len(case.tabs)
    before = _hip_det.CALLS['atomic']
    grads = hip.score_triples_bwd(CODE[case.kind], case.tabs, case.de, case.dr, case.h, case.t, case.r, case.go, (True,) * nt)
    assert _hip_det.CALLS['atomic'] - before == (nt if mode == 'rows' else 0), (case.tag, mode)
    return grads


def raw_bwd_atomic(hip, case, grads=None):
    """kge_score_triples_bwd's atomic mode through the C entry, into caller-zeroed tables."""
    nt = len(case.tabs)
    ga = [torch.zeros_like(x) for x in case.tabs] if grads is None else grads
    tb, g4 = list(case.tabs) + [None] * (4 - nt), ga + [None] * (4 - nt)
    rc = raw(hip.load_library(), 'kge_score_triples_bwd', CODE[case.kind], tb[0], tb[1], tb[2], tb[3], case.de, case.dr,
             case.h, case.t, case.r, case.h.shape[0], case.go, g4[0], g4[1], g4[2], g4[3], None, 0)
    return rc, ga


def raw_bwd_rows(hip, case, fill=float('nan'), pad=0):
    """The row mode through the C entry into a `fill`-ed rows buffer, then kge_segment_sum_rows per table.  Returns
    (rows viewed (streams, B, ld), gradient tables)."""
    lib = hip.load_library()
    kind, B, nt = case.kind, case.h.shape[0], len(case.tabs)
    ns, ld = N_STREAMS.get(kind, 3), case.de + pad
    rows = torch.full((ns * B, ld), fill, dtype=torch.float32, device=case.h.device)
    tb = list(case.tabs) + [None] * (4 - nt)
    rc = raw(lib, 'kge_score_triples_bwd', CODE[kind], tb[0], tb[1], tb[2], tb[3], case.de, case.dr, case.h, case.t, case.r,
             B, case.go, None, None, None, None, rows, ld)
    assert rc == 0, (case.tag, rc)
    grads = [torch.zeros_like(x) for x in case.tabs]
    for ti, s0, n_s, key in hip._BWD_STREAMS[CODE[kind]]:
        k0, n0, k1, n1 = (case.h, B, case.t, B) if key == 'ht' else (case.r, B, None, 0)
        perm = hip._key_perm(k0, k1, grads[ti].shape[0])
        rc = raw(lib, 'kge_segment_sum_rows', rows[s0 * B:], ld, grads[ti].shape[1], k0, n0, k1, n1, perm, grads[ti],
                 grads[ti].stride(0))
        assert rc == 0, (case.tag, 'kge_segment_sum_rows', ti, rc)
    return rows.view(ns, B, ld), grads


# ---------------------------------------------------------------------------
# 1. every bucket, both load paths, both backward modes
# ---------------------------------------------------------------------------
VEC4_WIDTHS = [4, 64, 256, 260, 512, 516, 1024]             # both sides of each NE boundary of the float4 path ...
SCALAR_WIDTHS = [1, 63, 65, 253, 257, 511, 513, 1023]       # ... and of the scalar path
TRANSD_PAIRS = [(72, 48), (300, 70), (516, 260), (1024, 4), (257, 257), (1023, 1)]


def bucket_cases():
    out = []
    for kind in KINDS:
        out += [pytest.param(kind, d, d, 0, id='%s-%d' % (kind, d)) for d in sorted(VEC4_WIDTHS + SCALAR_WIDTHS)]
        out.append(pytest.param(kind, 260, 260, 1, id='%s-260-one-float-off' % kind))
    out += [pytest.param('transd', de, dr, 0, id='transd-%d-%d' % (de, dr)) for de, dr in TRANSD_PAIRS]
    return out


@pytest.mark.parametrize('kind,de,dr,off', bucket_cases())
def test_every_row_width_bucket_forward_and_both_backward_modes(hip, monkeypatch, kind, de, dr, off):
    """B = 130 (33 blocks), n_ent = 50, n_rel = 5, skewed indices with a few h == t: the forward, the atomic backward
    (kinds below TORUSE_L1) and the row-mode backward through the Python wrappers at widths on both sides of every
    NE boundary of both load paths; TransD with d_rel ending in another 64-lane chunk / another NE bucket than d_ent."""
    tag = '%s d %d/%d%s' % (kind, de, dr, ' (tables one float off 16 bytes)' if off else '')
    case = make_case(kind, de, dr, 130, 50, 5, 7919 * CODE[kind] + 31 * de + dr + off, tag, off=off)
    assert bool((case.h == case.t).any())
    case.check_scores(hip.score_triples(CODE[kind], case.tabs, de, dr, case.h, case.t, case.r))
    for mode in (['atomic'] if CODE[kind] < hip.TORUSE_L1 else []) + ['rows']:
        case.check_grads(wrapper_bwd(hip, monkeypatch, case, mode), mode)


@pytest.mark.parametrize('d', [1025, 1028])
@pytest.mark.parametrize('kind', KINDS)
def test_rows_wider_than_1024_are_refused_and_nothing_is_written(hip, kind, d):
    """d = 1025 (scalar) and 1028 (float4): the C entry points return a non-zero code for the forward and for both
    backward modes, the Python wrappers raise, a sentinel-filled output / rows buffer / gradient tables keep every bit."""
    lib, code = hip.load_library(), CODE[kind]
    g = torch.Generator().manual_seed(d)
    tabs = [x.cuda() for x in make_tables(kind, d, d, g, 50, 5)]
    nt, B = len(tabs), 130
    h, t, r, go = (x.cuda() for x in make_triples(B, 50, 5, g))
    tb = tabs + [None] * (4 - nt)

    def sentinel(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)
    out, rows, ga = sentinel(B), sentinel(N_STREAMS.get(kind, 3) * B, d), [sentinel(*x.shape) for x in tabs]
    g4 = ga + [None] * (4 - nt)
    assert raw(lib, 'kge_score_triples', code, tb[0], tb[1], tb[2], tb[3], d, d, h, t, r, B, out) != 0
    assert raw(lib, 'kge_score_triples_bwd', code, tb[0], tb[1], tb[2], tb[3], d, d, h, t, r, B, go, g4[0], g4[1], g4[2], g4[3],
               None, 0) != 0
    assert raw(lib, 'kge_score_triples_bwd', code, tb[0], tb[1], tb[2], tb[3], d, d, h, t, r, B, go, None, None, None, None,
               rows, d) != 0
    with pytest.raises(RuntimeError):
        hip.score_triples(code, tabs, d, d, h, t, r)
    with pytest.raises(RuntimeError):
        hip.score_triples_bwd(code, tabs, d, d, h, t, r, go, (True,) * nt)
    torch.cuda.synchronize()
    for x in [out, rows] + ga:
        assert bool((bits(x) == SENTINEL).all())


# ---------------------------------------------------------------------------
# 2. past the grid cap
# ---------------------------------------------------------------------------
def grid_cap_batch():
    """Three full sweeps of the capped grid (KGE_K1_BLOCKS blocks of four wavefronts, 8192 by default) plus 777: a
    wavefront handles 3 or 4 triples -- every branch of the forward's pipeline (i1 < B, i2 < B, the break) and the
    backward's stride loop."""
    cap = int(os.environ.get('KGE_K1_BLOCKS', '0') or 0)
    return 3 * 4 * (cap if cap > 0 else 8192) + 777


BIG = {}


def big_case(kind, d):
    """The (kind, d) case of the grid-cap tests, computed once and shared by the forward and the backward test."""
    if (kind, d) not in BIG:
        dr = d if kind != 'transd' else (4 if d % 4 == 0 else 3)
        BIG[(kind, d)] = make_case(kind, d, dr, grid_cap_batch(), 3000, 11, 104729 * CODE[kind] + d,
                                   '%s d %d/%d B %d' % (kind, d, dr, grid_cap_batch()))
    return BIG[(kind, d)]


@pytest.mark.parametrize('d', [8, 5])
@pytest.mark.parametrize('kind', KINDS)
def test_forward_past_the_grid_cap_every_triple(hip, kind, d):
    case = big_case(kind, d)
    assert case.h.shape[0] > 4 * 8192 or 'KGE_K1_BLOCKS' in os.environ
    case.check_scores(hip.score_triples(CODE[kind], case.tabs, case.de, case.dr, case.h, case.t, case.r))
    if kind not in GRID_CAP_BWD_KINDS:
        BIG.pop((kind, d))


@pytest.mark.parametrize('d', [8, 5])
@pytest.mark.parametrize('kind', GRID_CAP_BWD_KINDS)
def test_backward_past_the_grid_cap_row_mode_and_atomic_mode(hip, kind, d):
    """The row mode with the default kge_segment_sum_rows reduction (the wrapper's own choice at this B) and the same
    call through the C entry in atomic mode (not TorusE, whose backward the wrapper never runs in that mode)."""
    from torchkge_amd import _hip_det
    case = big_case(kind, d)
    nt, B = len(case.tabs), case.h.shape[0]
    assert B >= hip.BWD_SORTED_MIN_BATCH
    before = _hip_det.CALLS['atomic']
    grads = hip.score_triples_bwd(CODE[kind], case.tabs, case.de, case.dr, case.h, case.t, case.r, case.go, (True,) * nt)
    assert _hip_det.CALLS['atomic'] - before == nt
    case.check_grads(grads, 'rows')
    if CODE[kind] < hip.TORUSE_L1:
        rc, ga = raw_bwd_atomic(hip, case)
        assert rc == 0
        case.check_grads(ga, 'atomic')
    BIG.pop((kind, d))


def test_segment_sum_rows_second_chunk_per_wavefront(hip):
    """M = 262144 + 33 sorted entries: the grid of 2048 blocks x 4 wavefronts x 32 entries is exhausted and wavefronts
    take a second chunk.  One key owns a quarter of the entries.  Bound: the forward bound of ANY fp32 summation order."""
    lib = hip.load_library()
    M, d, n_keys = 262144 + 33, 4, 700
    g = torch.Generator().manual_seed(23)
    keys = torch.randint(0, n_keys, (M,), generator=g)
    keys[torch.randperm(M, generator=g)[:M // 4]] = 17
    x = torch.randn(M, d, generator=g)
    keys, x = keys.cuda(), x.cuda()
    perm = torch.sort(keys, stable=True).indices
    n0 = M // 3
    out = torch.zeros(n_keys, d, device='cuda')
    assert raw(lib, 'kge_segment_sum_rows', x, d, d, keys[:n0].contiguous(), n0, keys[n0:].contiguous(), M - n0, perm, out, d) == 0
    n_run = torch.bincount(keys, minlength=n_keys).double().view(-1, 1)
    assert float(n_run.max()) * U < 0.01 and float(n_run.max()) >= M // 4
    sum64, abs64 = row_sum(n_keys, keys, x.double()), row_sum(n_keys, keys, x.double().abs())
    err, bound = (out.double() - sum64).abs(), 1.01 * n_run * U * abs64
    assert bool(torch.isfinite(out).all()) and bool((err <= bound).all()), float((err - bound).max())


# ---------------------------------------------------------------------------
# 3. kge_segment_sum_rows across its own buckets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 64, 65, 256, 257, 512, 513, 1024])
def test_segment_sum_rows_vs_float64_and_layout_contract(hip, d):
    """segment_sum_kernel<4 / 8 / 16> on the key cases of the ordered kernel's test, padded ld / out_ld with NaN in the
    pads, n1 == 0 and n1 > 0, into a zero and a non-zero `out`: what that test asserts of the ordered kernel."""
    lib = hip.load_library()
    g = torch.Generator().manual_seed(2000 + d)
    for name, keys, n_keys in key_cases():
        M = keys.shape[0]
        x = torch.randn(M, d, generator=g)
        perm = torch.sort(keys, stable=True).indices
        n_run = torch.bincount(keys, minlength=n_keys).double().view(-1, 1)
        sum64 = torch.zeros(n_keys, d, dtype=torch.float64).index_add_(0, keys, x.double())
        abs64 = torch.zeros(n_keys, d, dtype=torch.float64).index_add_(0, keys, x.double().abs())
        pattern = (torch.arange(n_keys * d, dtype=torch.float32).view(n_keys, d) % 13 - 6.25) * 0.37
        assert float(n_run.max()) * U < 0.01 and bool((n_run == 0).any())
        rows = nan_padded(x, 3)
        kd, pd = keys.cuda(), perm.cuda()
        for n0 in sorted({M, M // 3}):                      # n1 = 0 with k1 = NULL, and n1 > 0
            k0, k1 = kd[:n0].contiguous(), (kd[n0:].contiguous() if n0 < M else None)
            for fill in (torch.zeros(n_keys, d), pattern):
                out = nan_padded(fill, 5)
                before = out.clone()
                assert raw(lib, 'kge_segment_sum_rows', rows, d + 3, d, k0, n0, k1, M - n0, pd, out, d + 5) == 0
                got = out[:, :d].cpu()
                tag = (name, d, n0)
                assert torch.equal(bits(out[:, d:]), bits(before[:, d:])), tag         # the pads keep every bit
                absent = (n_run.view(-1) == 0).cuda()
                assert torch.equal(bits(out[absent]), bits(before[absent])), tag      # and so do rows of absent keys
                assert bool(torch.isfinite(got).all()), tag          # no pad column of `rows` reached a sum
                fill64 = fill.double()
                err = (got.double() - (fill64 + sum64)).abs()
                bound = 1.01 * n_run * U * (abs64 + fill64.abs())
                assert bool((err <= bound).all()), (tag, float((err - bound).max()))
                if not fill.any():                          # a run of one row is that row
                    one = (n_run.view(-1) == 1)
                    assert torch.equal(got[one], sum64[one].float()), tag


# ---------------------------------------------------------------------------
# 4. edges
# ---------------------------------------------------------------------------
def edge_dims(kind, d):
    return (d, d) if kind != 'transd' else (d, {8: 4, 260: 132}[d])     # (both on the float4 path)


ZERO_ROW = {0: 2, 1: 1, 2: 3, 3: 0}     # the all-zero row of table X (TransD's second entity table: row 4)


def zero_row(kind, X):
    return 4 if (kind, X) == ('transd', 2) else ZERO_ROW[X]


def clamped_case(kind, d):
    de, dr = edge_dims(kind, d)

    def edit(tabs, h, t, r, go):
        for X in NORMALISED[kind]:
            tabs[X][zero_row(kind, X)] = 0
        # a handful of triples on those rows (the rest of the batch is ordinary), head and tail side, also together
        h[10:14] = torch.tensor([2, 4, 7, 2])
        t[10:14] = torch.tensor([6, 9, 2, 4])
        t[14] = h[14] = 2
        r[20:24] = torch.tensor([0, 1, 3, 1])
        h[22], r[22] = 4, 3
    return make_case(kind, de, dr, 60, 12, 5, 100 + CODE[kind] * 10 + d, '%s d %d/%d zero rows' % (kind, de, dr), edit=edit)


@pytest.mark.parametrize('d', [8, 260])
@pytest.mark.parametrize('kind', ['transe_l1', 'transe_l2', 'distmult', 'transh', 'transd'])
def test_clamped_norms_all_zero_rows(hip, monkeypatch, kind, d):
    """One all-zero row in every table the kind normalises (1 / max(n, 1e-12) in the forward, g / n in normalize_bwd):
    scores finite and within TOL, gradients finite, the zero rows' gradients (~1e12 g) within GRAD_TOL of float64 on
    their own scale, every other row within its ordinary S_rho."""
    case = clamped_case(kind, d)
    de, dr = case.de, case.dr
    for X in NORMALISED[kind]:
        assert not bool(case.tabs[X][zero_row(kind, X)].any()) and bool(case.rows[X][2][zero_row(kind, X)])
    case.check_scores(hip.score_triples(CODE[kind], case.tabs, de, dr, case.h, case.t, case.r))
    for mode in ('atomic', 'rows'):
        grads = wrapper_bwd(hip, monkeypatch, case, mode)
        case.check_grads(grads, mode)
    # (TransH's norm_vect: with w^ = 0 every term of d score / d w^ carries a factor h.w^ = 0 or gd.w^ = 0)
    big = [float(grads[X][zero_row(kind, X)].abs().max()) for X in NORMALISED[kind] if (kind, X) != ('transh', 2)]
    assert min(big) > 1e6, big          # (the clamped gradients are of the size 1e12 g: the branch was taken)


EXACT = dict(e=7, r0=3, i0=5)


def exact_zero_case(kind, d):
    e, r0, i0 = EXACT['e'], EXACT['r0'], EXACT['i0']

    def edit(tabs, h, t, r, go):
        tabs[1][r0] = 0
        h[h == e], t[t == e], r[r == r0] = 0, 0, 0          # nothing else touches entity e and relation r0
        h[i0], t[i0], r[i0], go[i0] = e, e, r0, 1.5
    return make_case(kind, d, d, 40, 12, 5, 300 + CODE[kind] * 10 + d, '%s d %d exact zero' % (kind, d), edit=edit)


@pytest.mark.parametrize('d', [8, 260])
@pytest.mark.parametrize('kind', ['transe_l1', 'transe_l2', 'toruse_l1'])
def test_exact_zero_diff_gives_exact_zero_score_and_gradient_rows(hip, monkeypatch, kind, d):
    """A triple (e, e, r0) with R[r0] == 0: diff is zero in every element, the score is exactly 0 and so are its three
    gradient rows, in the tables of both modes and in the rows the row mode emits."""
    e, r0, i0 = EXACT['e'], EXACT['r0'], EXACT['i0']
    case = exact_zero_case(kind, d)
    assert float(case.go[i0]) == 1.5
    s = hip.score_triples(CODE[kind], case.tabs, d, d, case.h, case.t, case.r)
    case.check_scores(s)
    assert float(s[i0]) == 0.0
    for mode in (['atomic'] if CODE[kind] < hip.TORUSE_L1 else []) + ['rows']:
        grads = wrapper_bwd(hip, monkeypatch, case, mode)
        case.check_grads(grads, mode)
        assert not bool(grads[0][e].any()) and not bool(grads[1][r0].any()), mode
    rows, grads = raw_bwd_rows(hip, case, pad=3)
    case.check_grads(grads, 'rows (C entry)')
    assert not bool(rows[:, i0, :d].any())
    assert bool(torch.isnan(rows[:, :, d:]).all())          # the pad of the rows buffer is not written


def zero_go_case(kind, d):
    de, dr = edge_dims(kind, d)

    def edit(tabs, h, t, r, go):
        go[::3] = 0
    return make_case(kind, de, dr, 130, 50, 5, 500 + CODE[kind] * 10 + d, '%s d %d/%d go == 0' % (kind, de, dr), edit=edit)


@pytest.mark.parametrize('d', [8, 260])
@pytest.mark.parametrize('kind', KINDS)
def test_zero_grad_out_in_row_mode_writes_zero_rows(hip, kind, d):
    """go == 0 for a third of the batch, the rows buffer pre-filled with NaN: the kernel must still write those triples'
    rows (as zeros), so the reduced gradients are finite and equal the float64 reference of the same go.  Every kind:
    each is a kernel of its own, and the number of streams it fills comes from the kind's own row set."""
    case = zero_go_case(kind, d)
    assert int((case.go == 0).sum()) == 44
    rows, grads = raw_bwd_rows(hip, case)
    case.check_grads(grads, 'rows (C entry)')
    z = rows[:, case.go == 0]
    widths = [case.tabs[ti].shape[1] for ti, s0, n_s, key in hip._BWD_STREAMS[CODE[kind]] for _ in range(n_s)]
    streams = [s0 + j for ti, s0, n_s, key in hip._BWD_STREAMS[CODE[kind]] for j in range(n_s)]
    for st, w in zip(streams, widths):
        assert not bool(bits(z[st][:, :w]).any()), (kind, d, 'stream', st)
