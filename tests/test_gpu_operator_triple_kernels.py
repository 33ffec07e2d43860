"""GPU tests of the triple kernels of the five later model kinds (run with -m gpu on an MI355X): kge_score_triples /
kge_score_triples_bwd for RESCAL, HolE (bilinear_xform.hip) and TransR (transr_xform.hip) with kge_rescal_rel_grad /
kge_transr_rel_grad, kge_analogy_score_triples / _bwd (analogy.hip) and kge_convkb_prepare / kge_convkb_score_triples /
_bwd with the four layer gradients (convkb.hip) -- in every width bucket (the second pass of the 64-lane loops, the d = 512
edge of the LDS rows, every dv chunk of TransR's backward, both directions of TransR's rows_ld = max(d_e, d_r),
convkb_bwd_params_kernel's j stride past 256 and F + 1 = 513 blocks, 8 x 8 tiles of the per-relation reduction), past the
grid cap of 8192 blocks x 4 wavefronts (a second iteration of the grid-stride loops with their __syncthreads() and a partial
last group) and at the edges the code handles (clamped norms, h == t, go == 0, refused arguments).

Inputs, reference (float64 autograd with the gathered rows as leaves, on the device) and metric are those of
tests/test_operator_triples_host.py, which documents them and checks the inputs on the CPU; they are the ones
tests/test_gpu_triple_kernels.py applies to the ten kinds of score_triples.hip.  Every entry point is called through
helpers.raw with explicit leading dimensions: the rows buffer is a guarded_out view of leading dimension width + 3, each
stream may write its own width only (TransR: d_e columns in streams 0, 1, 3 and d_r in stream 2; ANALOGY d_sc + 2 d_c)
and every other element keeps its sentinel.

Gradient rows are checked per TRIPLE (|row - G[i, X]| <= GRAD_TOL scale_i) and per table row after kge_segment_sum_rows
(|got - ref| <= GRAD_TOL S_rho, rows no triple hits bit-zero).  The per-relation matrix gradients (rel_mat.grad,
proj_mat.grad) additionally meet the chain bound of tests/test_gpu_transr.py::test_rel_grad_reduction_tiles_and_segments
against the rows U, V the kernel wrote -- |gM - U64^T V64| <= n 2^-23 |U|^T |V| per relation of n triples -- and have the
same bits on a second run.  RESCAL's streams 2 / 3 (U = go h^, V = t^) and TransR's stream 3 (v = h^ - t^) are no
gradient of a table; they are compared with float64 directly: a normalised element is at most 1 in magnitude, its fp32
error at most ((d / 64 + 7) / 2 + 2) 2^-24 <= 10 * 2^-24 for d <= 512 (a lane's chain of d / 64 squares, six tree levels
and the last add, halved by the square root, the root's own rounding and the division), bound used: 16 * 2^-24 per
normalised element (x |go| for U, x 2 for v).

Both ratios are printed per (kind, shape, mode); DESIGN.md section 6 records the largest."""
import pytest
import torch

from tests.helpers import raw, guarded_out, assert_guard_intact
from tests.test_gpu_layout_contract import TRIPLE_KINDS, N_STREAMS, GRAD_TOL, KGE_EINVAL, KGE_EUNSUPPORTED
from tests.test_operator_triples_host import (OpCase, Spec, BUCKET_SPECS, GRID_SPECS, ZERO_ROW_SPECS, SAME_HT_SPECS,
                                              ZERO_GO_SPECS, ZERO_ROW, ZERO_AT, SAME_AT, N_ENT, stream_widths, bits)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF           # helpers.guarded_out's fp32 fill
NORM_TOL = 16 * 2.0 ** -24      # a normalised element against float64 (module docstring)
PAD = 3


@pytest.fixture(scope='module')
def libs():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip, _hip_analogy, _hip_convkb
    _hip.load_library()
    _hip_analogy.load_library()
    _hip_convkb.load_library()
    return _hip


CASES = {}


def get_case(spec):
    """The OpCase of a spec on the device, computed once."""
    if spec.id not in CASES:
        CASES[spec.id] = OpCase(spec, 'cuda')
    return CASES[spec.id]


def ids(specs):
    return [s.id for s in specs]


def sbits(x):
    """The memory of a (strided) fp32 view as int32."""
    return x.view(torch.int32)


# ---------------------------------------------------------------------------
# the entry points through raw()
# ---------------------------------------------------------------------------
def t3(tabs):
    """(pointer, leading dimension) x 3 of ANALOGY's (sc, re, im); a zero-width table passes NULL, 0."""
    out = []
    for x in tabs:
        out += [x, x.stride(0)] if x.shape[1] else [None, 0]
    return out


def dims_abi(case, dims=None):
    """(d_ent, d_rel) of kge_score_triples for the case's kind."""
    d = case.dims if dims is None else dims
    if case.kind == 'rescal':
        return d[0], d[0] * d[0]
    return (d[0], d[0]) if case.kind == 'hole' else (d[0], d[1])


class Run(object):
    """One forward and one row-mode backward of a case on the index vectors (h, t, r, go) -- the case's own, or the tiled
    ones of the grid-cap test -- into guarded outputs.  forward() / backward() take what the refusal tests vary: the widths
    passed to the entry point, the rows buffer and its leading dimension, the tables of the atomic mode."""

    def __init__(self, hip, case, h=None, t=None, r=None, go=None, tabs=None, params=None):
        self.hip, self.lib, self.case = hip, hip.load_library(), case
        self.tabs, self.params = case.tabs if tabs is None else tabs, case.params if params is None else params
        self.h, self.t, self.r, self.go = (case.h if h is None else h, case.t if t is None else t,
                                           case.r if r is None else r, case.go if go is None else go)
        self.B = self.h.shape[0]
        self.widths = stream_widths(case.kind, case.dims)
        self.W = max(self.widths)
        assert len(self.widths) == N_STREAMS.get(case.kind, 3)
        self.ws = None

    def prepare(self, dims=None, ws=None):
        """kge_convkb_prepare into a fresh workspace [wp | db | D | Dt] (sentinel-filled when `ws` is given)."""
        case = self.case
        d, F = case.dims if dims is None else dims
        w, cb, L, lb = self.params
        if ws is None:
            ws = torch.empty(4 * case.dims[1] + 4 + 2 * case.dims[0] * case.dims[1], device='cuda')
        rc = raw(self.lib, 'kge_convkb_prepare', w, cb, L, L.stride(0), lb, d, F, ws)
        self.ws = ws
        return rc

    def forward(self, out, dims=None):
        case, kind, tb = self.case, self.case.kind, self.tabs
        if kind in ('rescal', 'hole', 'transr'):
            de, dr = dims_abi(case, dims)
            tb = list(tb) + [None] * (4 - len(tb))
            return raw(self.lib, 'kge_score_triples', TRIPLE_KINDS.index(kind), tb[0], tb[1], tb[2], tb[3], de, dr, self.h,
                       self.t, self.r, self.B, out)
        d = case.dims if dims is None else dims
        if kind == 'analogy':
            return raw(self.lib, 'kge_analogy_score_triples', *(t3(tb[:3]) + t3(tb[3:]) + [d[0], d[1], self.h, self.t, self.r,
                                                                                            self.B, out]))
        return raw(self.lib, 'kge_convkb_score_triples', tb[0], tb[0].stride(0), tb[1], tb[1].stride(0), d[0], d[1], self.ws,
                   self.h, self.t, self.r, self.B, out)

    def backward(self, rows, ld, dims=None, atomic=None, s=None, g=None, par=(None, None, None, None)):
        case, kind, tb = self.case, self.case.kind, self.tabs
        if kind in ('rescal', 'hole', 'transr'):
            de, dr = dims_abi(case, dims)
            tb = list(tb) + [None] * (4 - len(tb))
            g0, g1 = atomic if atomic is not None else (None, None)
            return raw(self.lib, 'kge_score_triples_bwd', TRIPLE_KINDS.index(kind), tb[0], tb[1], tb[2], tb[3], de, dr, self.h,
                       self.t, self.r, self.B, self.go, g0, g1, None, None, rows, ld)
        d = case.dims if dims is None else dims
        if kind == 'analogy':
            return raw(self.lib, 'kge_analogy_score_triples_bwd', *(t3(tb[:3]) + t3(tb[3:]) + [d[0], d[1], self.h, self.t, self.r,
                                                                                                self.B, self.go, rows, ld]))
        return raw(self.lib, 'kge_convkb_score_triples_bwd', tb[0], tb[0].stride(0), tb[1], tb[1].stride(0), d[0], d[1], self.ws,
                   self.h, self.t, self.r, self.B, s, self.go, g, rows, ld, par[0], par[1], par[2], par[3])

    def run(self, with_params=True):
        """Forward into a guarded vector, backward into a guarded rows buffer of leading dimension W + 3 (ConvKB: and the
        four layer gradients into guarded buffers); every guard checked.  Returns self."""
        case, B = self.case, self.B
        if case.kind == 'convkb':
            assert self.prepare() == 0, case.tag
        self.out = guarded_out(B)
        assert self.forward(self.out) == 0, case.tag
        self.rows = guarded_out(len(self.widths) * B, self.W, PAD)
        self.ld = self.rows.stride(0)
        assert self.ld == self.W + PAD
        self.g, self.par, guards = None, [], []
        if case.kind == 'convkb':
            d, F = case.dims
            self.g = guarded_out(B)
            abi = []
            if with_params:     # the ABI's order (dL, dlb, dw, dcb); self.par in the order of case.params
                abi = [guarded_out(2, F * d), guarded_out(2), guarded_out(F, 3), guarded_out(F)]
                self.par = [abi[2].reshape(F, 3, 1), abi[3], abi[0], abi[1]]
            s = self.out.clone()
            assert self.backward(self.rows, self.ld, s=s, g=self.g, par=abi or (None,) * 4) == 0, case.tag
            guards = abi
        else:
            assert self.backward(self.rows, self.ld) == 0, case.tag
        torch.cuda.synchronize()
        for v in [self.out, self.rows] + ([self.g] if self.g is not None else []) + guards:
            assert_guard_intact(v)
        self.streams = self.rows.as_strided((len(self.widths), B, self.W), (B * self.ld, self.ld, 1), self.rows.storage_offset())
        for st, w in enumerate(self.widths):                # each stream writes its own width and nothing beside it
            assert bool((sbits(self.streams[st][:, w:]) == SENTINEL).all()), (case.tag, 'stream', st, 'wrote past its width')
        return self

    def table_rows(self, X):
        """The gradient rows of table X: (2B, w) for an entity table (h's rows, then t's), (B, w) for a relation table."""
        key, streams, c0, w = self.case.layout[X]
        return torch.cat([self.streams[st][:, c0:c0 + w] for st in streams])

    def reduce(self, X):
        """kge_segment_sum_rows of table X's streams, read in place from the padded rows buffer."""
        case, B, hip = self.case, self.B, self.hip
        key, streams, c0, w = case.layout[X]
        n = case.tabs[X].shape[0]
        gt = guarded_out(n, w, 2)
        gt.zero_()
        k0, n0, k1, n1 = (self.h, B, self.t, B) if key == 'ht' else (self.r, B, None, 0)
        perm = hip._key_perm(k0, k1, n)
        src = self.rows[streams[0] * B:, c0:]
        assert raw(self.lib, 'kge_segment_sum_rows', src, self.ld, w, k0, n0, k1, n1, perm, gt, gt.stride(0)) == 0, (case.tag, X)
        torch.cuda.synchronize()
        assert_guard_intact(gt)
        return gt.contiguous()

    def rel_grad(self, X):
        """kge_rescal_rel_grad / kge_transr_rel_grad on the U and V streams the backward wrote (perm from _key_perm)."""
        case, B = self.case, self.B
        n_rel, w = case.tabs[X].shape
        gM = torch.full((n_rel, w), float('nan'), device='cuda')
        perm = self.hip._key_perm(self.r, None, n_rel)
        U, V = self.rows[2 * B:], self.rows[3 * B:]
        if case.kind == 'rescal':
            rc = raw(self.lib, 'kge_rescal_rel_grad', U, V, self.ld, case.dims[0], self.r, perm, B, n_rel, gM, gM.stride(0))
        else:
            rc = raw(self.lib, 'kge_transr_rel_grad', U, self.ld, V, self.ld, case.dims[1], case.dims[0], self.r, perm, B, n_rel,
                     gM, gM.stride(0))
        assert rc == 0, (case.tag, rc)
        return gM

    def check_rel_grad(self, X):
        """The chain bound against the kernel's own U, V rows, the same bits on two runs.  Returns gM."""
        case = self.case
        gM = self.rel_grad(X)
        assert torch.equal(bits(self.rel_grad(X)), bits(gM)), (case.tag, 'matrix gradient: other bits on a second run')
        assert bool(torch.isfinite(gM).all()), case.tag
        d_u, d_v = (case.dims[0], case.dims[0]) if case.kind == 'rescal' else (case.dims[1], case.dims[0])
        U64, V64 = self.streams[2][:, :d_u].double(), self.streams[3][:, :d_v].double()
        got = gM.double().view(-1, d_u, d_v)
        for rho in range(gM.shape[0]):
            sel = self.r == rho
            n = int(sel.sum())
            ref = U64[sel].t() @ V64[sel]
            bound = n * 2.0 ** -23 * (U64[sel].abs().t() @ V64[sel].abs())
            err = (got[rho] - ref).abs()
            assert bool((err <= bound).all()), (case.tag, 'relation', rho, n, float((err - bound).max()))
            if n == 0:
                assert not bool(bits(gM[rho]).any()), (case.tag, 'relation', rho)
        return gM


def check_operand_streams(run, case):
    """RESCAL's U = go h^ and V = t^, TransR's v = h^ - t^ against float64 (module docstring)."""
    if case.kind not in ('rescal', 'transr'):
        return
    E = case.tabs[0].double()
    hn = E[case.h] / E[case.h].norm(dim=1, keepdim=True).clamp_min(1e-12)
    tn = E[case.t] / E[case.t].norm(dim=1, keepdim=True).clamp_min(1e-12)
    d = case.dims[0]
    if case.kind == 'rescal':
        ago = case.go.abs().double().view(-1, 1)
        assert bool(((run.streams[2][:, :d].double() - case.go.double().view(-1, 1) * hn).abs() <= NORM_TOL * ago).all()), case.tag
        assert bool(((run.streams[3][:, :d].double() - tn).abs() <= NORM_TOL).all()), case.tag
    else:
        assert bool(((run.streams[3][:, :d].double() - (hn - tn)).abs() <= 2 * NORM_TOL).all()), case.tag


def check_case(hip, case, mode='rows'):
    """Forward, row-mode backward, the reductions: everything the bucket test asserts of one case.  Returns the Run."""
    run = Run(hip, case).run()
    q = case.score_ratio(run.out)
    print('operator triples %s scores: max |s - float64| / bound %.3g' % (case.tag, q))
    assert q <= 1.0, (case.tag, 'scores', q)
    tri, tab = [], []
    for X, (key, streams, c0, w) in enumerate(case.layout):
        if w == 0:
            continue
        if streams is None:
            tab.append(case.ratio(X, run.check_rel_grad(X)))
            continue
        tri.append(case.tri_ratio(X, run.table_rows(X)))
        tab.append(case.ratio(X, run.reduce(X)))
    par = [case.param_ratio(k, x) for k, x in enumerate(run.par)]
    print('operator triples %s %s: max |grad - float64| / scale per triple %s, / S_row per table %s, fp32 restatement %s%s'
          % (case.tag, mode, ' '.join('%.3g' % x for x in tri), ' '.join('%.3g' % x for x in tab),
             ' '.join('%.3g' % x for x in case.ratio32),
             '; layer gradients / bound %s (restatement %s)' % (' '.join('%.3g' % x for x in par),
                                                               ' '.join('%.3g' % x for x in case.param32)) if par else ''))
    assert max(tri) <= GRAD_TOL and max(tab) <= GRAD_TOL, (case.tag, mode, tri, tab)
    assert max(par + [0.0]) <= 1.0, (case.tag, 'layer gradients', par)
    check_operand_streams(run, case)
    return run


def hole_atomic(hip, case):
    """HolE's atomic mode into zeroed, guarded tables: the same metric, untouched rows bit-zero (OpCase.ratio)."""
    run = Run(hip, case)
    ga = [guarded_out(x.shape[0], x.shape[1]) for x in case.tabs]
    for x in ga:
        x.zero_()
    assert run.backward(None, 0, atomic=ga) == 0, case.tag
    torch.cuda.synchronize()
    q = [case.ratio(X, x.contiguous()) for X, x in enumerate(ga)]
    print('operator triples %s atomic: max |grad - float64| / S_row per table %s' % (case.tag, ' '.join('%.3g' % x for x in q)))
    assert max(q) <= GRAD_TOL, (case.tag, 'atomic', q)
    for x in ga:
        assert_guard_intact(x)


# ---------------------------------------------------------------------------
# 1. every width bucket, forward and backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('spec', BUCKET_SPECS, ids=ids(BUCKET_SPECS))
def test_every_width_bucket_forward_and_backward(libs, spec):
    """B = 203 (widths <= 129) or 37, 50 entities, 5 relations, three quarters of the batch on one head and one relation,
    a few h == t: scores, gradient rows per stream, the reduced table gradients and the matrix gradients against float64;
    the rows buffer has leading dimension width + 3 and every element outside a stream's own width keeps its sentinel.
    HolE also in atomic mode."""
    case = get_case(spec)
    assert bool((case.h == case.t).any()) and case.B % 4 != 0
    check_case(libs, case)
    if spec.kind == 'hole':
        hole_atomic(libs, case)
    CASES.pop(spec.id)


# ---------------------------------------------------------------------------
# 2. past the grid cap
# ---------------------------------------------------------------------------
def grid_cap_batch():
    """Two full sweeps of the capped grid (8192 blocks of four wavefronts, KGE_K1_BLOCKS for the classic kinds only) plus
    3: every block takes a second iteration of its grid-stride loop, the last group is partial."""
    return 2 * 4 * 8192 + 3


@pytest.mark.parametrize('spec', GRID_SPECS, ids=ids(GRID_SPECS))
def test_past_the_grid_cap_results_depend_on_the_triple_only(libs, spec):
    """B = 65539 tiled from 97 triples (i mod 97, go alike): every score and every gradient row of every stream equals,
    bit for bit, entry i mod 97 of a separate B = 97 run, which alone is compared with float64.  The matrix gradients over
    segments of about 21 846 triples meet the chain bound with the same bits on two runs; ConvKB's four layer gradients
    meet the metric of tests/test_gpu_convkb.py::test_backward_vs_float64_autograd with the same bits on two runs."""
    from tests import convkb_ref as cr
    case = get_case(spec)
    base = check_case(libs, case)
    B = grid_cap_batch()
    idx = torch.arange(B, device='cuda') % case.B
    big = Run(libs, case, case.h[idx].contiguous(), case.t[idx].contiguous(), case.r[idx].contiguous(),
              case.go[idx].contiguous()).run()
    assert torch.equal(bits(big.out), bits(base.out)[idx]), (case.tag, 'a score depends on the position in the batch')
    for st in range(len(big.widths)):
        assert torch.equal(bits(big.streams[st]), bits(base.streams[st])[idx]), (case.tag, 'stream', st)
    if case.kind == 'convkb':
        assert torch.equal(bits(big.g), bits(base.g)[idx]), case.tag
        again = Run(libs, case, big.h, big.t, big.r, big.go).run()
        for a, b in zip(big.par, again.par):
            assert torch.equal(bits(a), bits(b)), (case.tag, 'layer gradients: other bits on a second run')
        p64 = [x.detach().double().requires_grad_(True) for x in case.params]
        s64 = cr.sf64([x.double() for x in case.tabs] + p64, big.h, big.t, big.r)
        (s64 * big.go.double()).sum().backward()
        for k, (got, ref) in enumerate(zip(big.par, p64)):
            err = float((got.double() - ref.grad).abs().max())
            bound = 1e-4 * max(1.0, float(ref.grad.abs().max()))
            print('operator triples %s B %d layer gradient %d: max err %.3g (bound %.3g)' % (case.tag, B, k, err, bound))
            assert got.shape == ref.grad.shape and err < bound, (case.tag, k, err, bound)
    for X, (key, streams, c0, w) in enumerate(case.layout):
        if streams is None:
            big.check_rel_grad(X)
    CASES.pop(spec.id)


# ---------------------------------------------------------------------------
# 3. edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('spec', ZERO_ROW_SPECS, ids=ids(ZERO_ROW_SPECS))
def test_clamped_norms_all_zero_entity_row(libs, spec):
    """An all-zero entity row as h, as t and as both (1 / max(n, 1e-12) forward, g / n backward): scores within TOL,
    the zero row's gradient rows (~1e12 g) within GRAD_TOL of float64 on their own scale."""
    case = get_case(spec)
    assert not bool(case.tabs[0][ZERO_ROW].any())
    assert case.h[ZERO_AT:ZERO_AT + 3].tolist() == [ZERO_ROW, 4, ZERO_ROW] and case.t[ZERO_AT:ZERO_AT + 3].tolist() == [6, ZERO_ROW, ZERO_ROW]
    run = check_case(libs, case)
    if spec.kind == 'hole':
        hole_atomic(libs, case)
    d = case.dims[0]
    big = [float(run.streams[0][ZERO_AT, :d].abs().max()), float(run.streams[1][ZERO_AT + 1, :d].abs().max())]
    assert min(big) > 1e6, big          # (the clamped gradients are of the size 1e12 g: the branch was taken)
    CASES.pop(spec.id)


@pytest.mark.parametrize('spec', SAME_HT_SPECS, ids=ids(SAME_HT_SPECS))
def test_transr_same_head_and_tail_gives_exact_zero_v(libs, spec):
    """h == t: v = h^ - t^ is exactly 0, so two such triples of one relation and different entities have the same score
    bits, and the d t row is the exact negation of the d h row, bit for bit."""
    case = get_case(spec)
    i, j = SAME_AT, SAME_AT + 1
    assert int(case.h[i]) == int(case.t[i]) != int(case.h[j]) == int(case.t[j]) and int(case.r[i]) == int(case.r[j])
    assert float(case.go[i]) != 0 and float(case.go[j]) != 0
    run = check_case(libs, case)
    d = case.dims[0]
    assert torch.equal(bits(run.out[i:i + 1]), bits(run.out[j:j + 1]))
    same = case.h == case.t
    assert int(same.sum()) >= 2
    assert not bool(run.streams[3][same][:, :d].any())
    dh, dt = run.streams[0][same][:, :d], run.streams[1][same][:, :d]
    assert bool(dh.any()) and torch.equal(bits(dt), bits(-dh))
    CASES.pop(spec.id)


@pytest.mark.parametrize('spec', ZERO_GO_SPECS, ids=ids(ZERO_GO_SPECS))
def test_zero_grad_out_in_row_mode_writes_zero_rows(libs, spec):
    """go == 0 for a third of the batch, the rows buffer pre-filled with NaN sentinels: the kernel still writes those
    triples' rows, as zeros (streams 0 - 2 of RESCAL, HolE and TransR, every stream of ANALOGY and ConvKB); stream 3 holds
    t^ / v whatever go is and is compared with float64 (check_operand_streams)."""
    case = get_case(spec)
    assert int((case.go == 0).sum()) >= 44
    run = check_case(libs, case)
    z = case.go == 0
    for st, w in enumerate(run.widths[:3]):
        assert bool((run.streams[st][z][:, :w] == 0).all()), (case.tag, 'stream', st)
    if case.kind == 'convkb':
        assert bool((run.g[z] == 0).all())
    CASES.pop(spec.id)


def wide_inputs(kind, dims, n_rel):
    """Zero tables (and ConvKB layer parameters) of a width the entry points refuse: every pointer is valid for the width
    it is passed with, so that the call is well-formed whatever the entry point does with it."""
    def Z(*shape):
        return torch.zeros(*shape, device='cuda')
    if kind in ('rescal', 'hole'):
        return [Z(N_ENT, dims[0]), Z(n_rel, dims[0] * dims[0] if kind == 'rescal' else dims[0])], []
    if kind == 'transr':
        return [Z(N_ENT, dims[0]), Z(n_rel, dims[1]), Z(n_rel, dims[0] * dims[1])], []
    if kind == 'analogy':
        return [Z(n, w) for n in (N_ENT, n_rel) for w in (dims[0], dims[1], dims[1])], []
    d, F = dims
    return [Z(N_ENT, d), Z(n_rel, d)], [Z(F, 3, 1), Z(F), Z(2, F * d), Z(2)]


WIDE = {'rescal': [((513,), KGE_EINVAL)], 'hole': [((513,), KGE_EINVAL)],
        'transr': [((513, 3), KGE_EUNSUPPORTED), ((3, 513), KGE_EUNSUPPORTED)],
        'analogy': [((513, 0), KGE_EUNSUPPORTED), ((0, 513), KGE_EUNSUPPORTED)],
        'convkb': [((513, 1), KGE_EUNSUPPORTED), ((1, 513), KGE_EUNSUPPORTED)]}


@pytest.mark.parametrize('kind', ['rescal', 'hole', 'transr', 'analogy', 'convkb'])
def test_refusals_write_nothing(libs, kind):
    """The codes the headers document, with outputs, rows and layer gradients in sentinel-filled buffers that keep every
    bit: widths past 512, RESCAL's d_rel != d^2, RESCAL / TransR backward without rows, rows_ld one below the width
    (TransR: below max(d_e, d_r) in both directions)."""
    spec = {s.kind: s for s in ZERO_GO_SPECS if max(s.dims) <= 8}[kind]
    case = get_case(spec)
    run = Run(libs, case)
    B, ns = run.B, len(run.widths)
    out, rows, g = guarded_out(B), guarded_out(ns * B, 520, PAD), guarded_out(B)
    ld = rows.stride(0)
    par = [guarded_out(2, 513), guarded_out(2), guarded_out(513, 3), guarded_out(513)] if kind == 'convkb' else []
    par4 = par or (None,) * 4
    s = torch.full((B,), 0.5, device='cuda')
    for dims, code in WIDE[kind]:
        tabs, params = wide_inputs(kind, dims, spec.n_rel)
        wrun = Run(libs, case, tabs=tabs, params=params)
        if kind == 'convkb':
            ws = guarded_out(8192)
            assert wrun.prepare(dims, ws=ws) == code, (kind, dims)
            torch.cuda.synchronize()
            assert_guard_intact(ws, rows=0)
        assert wrun.forward(out, dims) == code, (kind, dims)
        assert wrun.backward(rows, ld, dims, s=s, g=g, par=par4) == code, (kind, dims)
    d = case.dims
    if kind == 'convkb':
        assert run.prepare() == 0
    if kind == 'rescal':
        lib, tb, code = run.lib, case.tabs, TRIPLE_KINDS.index(kind)
        for d_rel in (d[0] * d[0] - 1, d[0]):
            assert raw(lib, 'kge_score_triples', code, tb[0], tb[1], None, None, d[0], d_rel, run.h, run.t, run.r, B, out) == KGE_EINVAL
            assert raw(lib, 'kge_score_triples_bwd', code, tb[0], tb[1], None, None, d[0], d_rel, run.h, run.t, run.r, B, run.go,
                       None, None, None, None, rows, ld) == KGE_EINVAL
    if kind in ('rescal', 'transr'):        # no atomic mode: the matrix gradient exists only through the row streams
        ga = [guarded_out(x.shape[0], x.shape[1]) for x in case.tabs[:2]]
        assert run.backward(None, 0, atomic=ga) == KGE_EINVAL
        assert run.backward(None, ld, atomic=ga) == KGE_EINVAL
        torch.cuda.synchronize()
        for x in ga:
            assert_guard_intact(x, rows=0)
    assert run.backward(rows, run.W - 1, s=s, g=g, par=par4) == KGE_EINVAL, kind
    if kind == 'transr':                    # (8, 5) and its transpose: d_e - 1 and d_r - 1 are both below the width
        assert run.backward(rows, d[1]) == KGE_EINVAL
        flip = Run(libs, get_case(Spec('transr', (d[1], d[0]), spec.B, 'zero_go')))
        assert flip.W == run.W and flip.backward(rows, run.W - 1) == KGE_EINVAL and flip.backward(rows, d[1]) == KGE_EINVAL
    torch.cuda.synchronize()
    for v in [out, rows, g] + par:
        assert_guard_intact(v, rows=0)
    CASES.clear()
