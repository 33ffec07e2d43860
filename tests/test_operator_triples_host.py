"""CPU companion of tests/test_gpu_operator_triple_kernels.py: the inputs, the float64 reference and the metric of the
triple kernels of RESCAL / HolE (bilinear_xform.hip), TransR (transr_xform.hip), ANALOGY (analogy.hip) and ConvKB
(convkb.hip), and the checks ON THE INPUTS, which run here without a GPU for every shape the GPU file runs.

Reference and metric are those of tests/test_gpu_triple_kernels.py: float64 autograd with the GATHERED rows as leaves (for
RESCAL and TransR the gathered per-relation matrix rows too), so that G[i, X] -- triple i's gradient row for table X --
exists on its own; per table X, m_X = max over triples (go_i != 0, no clamped row) of max |G[i, X]| / |go_i|; a triple's
scale is |go_i| m_X, or max |G[i, X]| where the stream's own row is all-zero; S_rho = the sum of the scales of the triples
that hit row rho; |got - ref| <= GRAD_TOL S_rho elementwise, rows no triple hits are bit-zero; a normalised row of width 1
has the exact-zero reference.  Scores: |s - s64| <= TOL max(1, |s64|).

What OpCase asserts of the inputs, for every spec of SPECS (this file runs them on the CPU, the GPU file builds the same
cases on the device):
  * the fp32 ATen restatement of the scores is within a quarter of the score bound;
  * its gradient ratio max |x - ref| / S_rho is at most GRAD_TOL / 10 (ConvKB's four layer gradients: a tenth of the
    bound of tests/test_gpu_convkb.py::test_backward_vs_float64_autograd);
  * ConvKB: |z| <= 4 in float64 (s (1 - s) keeps the gradient's digits), and at most 3 % of the batch lies inside the ReLU
    kink band -- a triple with some (f, j) where |v64| < 8 * 2^-24 (|w0 x0| + |w1 x1| + |w2 x2| + |cb|): fp32 may see the
    other side of the ReLU there (the TransE-L1 rule of tests/test_gpu_triple_kernels.py); go_i is set to 0 for those triples
    BEFORE anything runs.
If a shape fails one of them the inputs are wrong, not the bound.

Inputs: RESCAL / HolE entity rows randn * 0.5, relation rows randn (h^ . B_r . t^ is then O(1): |s64| <= 3 or so);
TransR random_tables of tests/test_gpu_transr.py; ANALOGY random_tables of tests/test_gpu_analogy.py at scale
0.5 min(1, (16 / K)^(1/3)), K = d_sc + 2 d_c, so that the sum of |terms| of a score stays O(1) up to K = 1536; ConvKB
rand_params of tests/test_gpu_convkb.py with the gain that puts the batch's largest |z - db| at 3 (at most 3)."""
import math

import pytest
import torch

from tests import analogy_ref as ar
from tests import convkb_ref as cr
from tests.test_gpu_analogy import random_tables as analogy_tables
from tests.test_gpu_convkb import rand_params
from tests.test_gpu_deterministic import skewed_triples
from tests.test_gpu_layout_contract import GRAD_TOL, TOL, triple_sf64
from tests.test_gpu_transr import random_tables as transr_tables

N_ENT, N_REL = 50, 5
PARAM_TOL = 1e-4        # x max(1, |grad|max): GRAD_TOL of tests/test_gpu_convkb.py::test_backward_vs_float64_autograd
KINK = 8 * 2.0 ** -24
NORMALISED = {'rescal': (0,), 'hole': (0,), 'transr': (0,)}     # the tables whose gathered rows are normalised


class Spec(object):
    """One case: kind, dims ((d,), (d_e, d_r), (d_sc, d_c) or (d, F)), batch, variant (None: skewed triples with a few
    h == t; 'grid': the 97 base triples of the grid-cap test; 'zero_rows', 'same_ht', 'zero_go': the edges)."""

    def __init__(self, kind, dims, B, variant=None, n_rel=N_REL):
        self.kind, self.dims, self.B, self.variant, self.n_rel = kind, tuple(dims), B, variant, n_rel
        self.id = '%s-%s%s' % (kind, 'x'.join(str(x) for x in dims), '-' + variant if variant else '')
        self.seed = 7919 * KINDS.index(kind) + 31 * dims[0] + dims[-1] + 1000003 * (VARIANTS.index(variant) + 1)


KINDS = ['rescal', 'hole', 'transr', 'analogy', 'convkb']
VARIANTS = [None, 'grid', 'zero_rows', 'same_ht', 'zero_go']
WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 257, 511, 512]
BUCKET_DIMS = {
    'rescal': [(d,) for d in WIDTHS],
    'hole': [(d,) for d in WIDTHS],
    'transr': [(1, 1), (1, 512), (512, 1), (63, 65), (64, 64), (65, 63), (129, 257), (257, 129), (448, 5), (449, 5), (511, 512),
               (512, 511), (512, 512)],
    'analogy': [(0, 1), (1, 0), (63, 65), (64, 64), (65, 63), (257, 129), (0, 512), (512, 0), (512, 512)],
    'convkb': [(1, 1), (63, 2), (64, 3), (65, 1), (255, 2), (256, 1), (257, 3), (512, 2), (2, 512), (3, 257), (33, 64)],
}
GRID_DIMS = {'rescal': (5,), 'hole': (5,), 'transr': (5, 3), 'analogy': (2, 3), 'convkb': (3, 2)}
EDGE_DIMS = {'rescal': [(8,), (260,)], 'hole': [(8,), (260,)], 'transr': [(8, 5), (260, 132)], 'analogy': [(8, 4), (260, 130)],
             'convkb': [(8, 3), (260, 2)]}


def bucket_batch(dims):
    """203 for widths <= 129, 37 above: both leave a partial last block of four triples."""
    return 203 if max(dims) <= 129 else 37


BUCKET_SPECS = [Spec(k, dims, bucket_batch(dims)) for k in KINDS for dims in BUCKET_DIMS[k]]
GRID_SPECS = [Spec(k, GRID_DIMS[k], 97, 'grid', n_rel=4) for k in KINDS]      # (relation 3 is never hit)
ZERO_ROW_SPECS = [Spec(k, dims, 61, 'zero_rows') for k in ('rescal', 'hole', 'transr') for dims in EDGE_DIMS[k]]
SAME_HT_SPECS = [Spec('transr', dims, 61, 'same_ht') for dims in EDGE_DIMS['transr']]
ZERO_GO_SPECS = [Spec(k, dims, 130, 'zero_go') for k in KINDS for dims in EDGE_DIMS[k]]
SPECS = BUCKET_SPECS + GRID_SPECS + ZERO_ROW_SPECS + SAME_HT_SPECS + ZERO_GO_SPECS
ZERO_ROW, ZERO_AT = 2, 10       # the all-zero entity row; triples ZERO_AT .. + 2 have it as h, as t, as both
SAME_AT = 20                    # triples SAME_AT, SAME_AT + 1 of 'same_ht': h == t, one relation, different entities


def table_layout(kind, dims):
    """Per table: (key 'ht' | 'r', the streams of the rows buffer that hold its gradient rows -- None: the per-relation
    matrix, reduced from streams 2 / 3 by kge_rescal_rel_grad / kge_transr_rel_grad --, first column, width)."""
    if kind == 'rescal':
        return [('ht', (0, 1), 0, dims[0]), ('r', None, 0, dims[0] * dims[0])]
    if kind == 'hole':
        return [('ht', (0, 1), 0, dims[0]), ('r', (2,), 0, dims[0])]
    if kind == 'transr':
        return [('ht', (0, 1), 0, dims[0]), ('r', (2,), 0, dims[1]), ('r', None, 0, dims[0] * dims[1])]
    if kind == 'analogy':
        a, c = dims
        return [('ht', (0, 1), 0, a), ('ht', (0, 1), a, c), ('ht', (0, 1), a + c, c), ('r', (2,), 0, a), ('r', (2,), a, c),
                ('r', (2,), a + c, c)]
    return [('ht', (0, 1), 0, dims[0]), ('r', (2,), 0, dims[0])]


def stream_widths(kind, dims):
    """The columns each stream of the row mode may write."""
    if kind == 'rescal':
        return [dims[0]] * 4
    if kind == 'transr':
        return [dims[0], dims[0], dims[1], dims[0]]
    if kind == 'analogy':
        return [dims[0] + 2 * dims[1]] * 3
    return [dims[0]] * 3


def analogy_scale(dims):
    return 0.5 * min(1.0, (16.0 / (dims[0] + 2 * dims[1])) ** (1.0 / 3.0))


def bilinear_sf(kind, E, rel, d, h, t, r):
    """tests/test_gpu_rescal_hole.py::sf64 without the upcast: the restatement in the dtype of its arguments."""
    hn = E[h] / E[h].norm(dim=1, keepdim=True).clamp_min(1e-12)
    tn = E[t] / E[t].norm(dim=1, keepdim=True).clamp_min(1e-12)
    if kind == 'rescal':
        ops = rel.view(-1, d, d)
    else:
        i = torch.arange(d, device=rel.device).view(d, 1)
        j = torch.arange(d, device=rel.device).view(1, d)
        ops = rel[:, (j - i) % d]
    return torch.einsum('bi,bij,bj->b', hn, ops[r], tn)


def analogy_sf(tabs, h, t, r):
    """tests/analogy_ref.py::sf64 without the upcast."""
    a, b, c, d, e, f = tabs[0][h], tabs[1][h], tabs[2][h], tabs[3][r], tabs[4][r], tabs[5][r]
    q = torch.cat([a * d, b * e - c * f, b * f + c * e], dim=1)
    return (q * torch.cat([tabs[0][t], tabs[1][t], tabs[2][t]], dim=1)).sum(dim=1)


def convkb_v(params, x0, x1, x2):
    """v[i, f, j] of tests/convkb_ref.py in the dtype of its arguments."""
    w = params[2].reshape(params[2].shape[0], 3)
    return (w[:, 0, None] * x0.unsqueeze(-2) + w[:, 1, None] * x1.unsqueeze(-2) + w[:, 2, None] * x2.unsqueeze(-2)
            + params[3][:, None])


def convkb_z(params, x0, x1, x2):
    D = (params[4][1] - params[4][0]).reshape(params[2].shape[0], -1)
    return (D * torch.relu(convkb_v(params, x0, x1, x2))).sum(dim=(-2, -1)) + (params[5][1] - params[5][0])


def convkb_sf(params, h, t, r):
    """tests/convkb_ref.py::sf64 without the upcast."""
    return torch.sigmoid(convkb_z(params, params[0][h], params[1][r], params[0][t]))


def convkb_kinks(params, h, t, r):
    """The triples with some (f, j) inside the band where fp32 may take the other side of the ReLU."""
    p = [x.double() for x in params]
    x0, x1, x2 = p[0][h], p[1][r], p[0][t]
    w = p[2].reshape(-1, 3)
    mag = ((w[:, 0, None] * x0.unsqueeze(-2)).abs() + (w[:, 1, None] * x1.unsqueeze(-2)).abs()
           + (w[:, 2, None] * x2.unsqueeze(-2)).abs() + p[3][:, None].abs())
    return (convkb_v(p, x0, x1, x2).abs() < KINK * mag).flatten(1).any(1)


def make_inputs(spec):
    """(tables, layer parameters, h, t, r, go) on the CPU."""
    kind, dims, B, n_rel = spec.kind, spec.dims, spec.B, spec.n_rel
    g = torch.Generator().manual_seed(spec.seed)
    h, t, r, go = skewed_triples(B, N_ENT, n_rel, g)
    t[0] = h[0]
    t[B - 7:B - 3] = h[B - 7:B - 3]         # a few h == t, the hub included
    if spec.variant == 'grid':
        r = torch.arange(B) % (n_rel - 1)   # the tiled batch then has three segments of about 21 846 triples
    elif spec.variant == 'zero_rows':
        h[ZERO_AT:ZERO_AT + 3] = torch.tensor([ZERO_ROW, 4, ZERO_ROW])
        t[ZERO_AT:ZERO_AT + 3] = torch.tensor([6, ZERO_ROW, ZERO_ROW])
    elif spec.variant == 'same_ht':
        h[SAME_AT:SAME_AT + 2] = t[SAME_AT:SAME_AT + 2] = torch.tensor([7, 9])
        r[SAME_AT:SAME_AT + 2] = 1
    elif spec.variant == 'zero_go':
        go[::3] = 0
    params = []
    if kind in ('rescal', 'hole'):
        d = dims[0]
        tabs = [torch.randn(N_ENT, d, generator=g) * 0.5, torch.randn(n_rel, d * d if kind == 'rescal' else d, generator=g)]
    elif kind == 'transr':
        tabs = list(transr_tables(N_ENT, n_rel, dims[0], dims[1], spec.seed))
    elif kind == 'analogy':
        tabs = analogy_tables(N_ENT, n_rel, dims[0], dims[1], g, analogy_scale(dims))
    else:
        p = rand_params(N_ENT, n_rel, dims[0], dims[1], torch.Generator().manual_seed(spec.seed + 1))
        z1 = convkb_z([x.double() for x in p], p[0].double()[h], p[1].double()[r], p[0].double()[t]) - (p[5][1] - p[5][0]).double()
        gain = float('%.3g' % min(3.0, 3.0 / max(float(z1.abs().max()), 1e-30)))
        p = rand_params(N_ENT, n_rel, dims[0], dims[1], torch.Generator().manual_seed(spec.seed + 1), gain=gain)
        tabs, params = p[:2], p[2:]
    if spec.variant == 'zero_rows':
        tabs[0][ZERO_ROW] = 0
    return tabs, params, h, t, r, go


def row_sum(n, keys, vals):
    """zeros(n, ...).index_add_(0, keys, vals) in vals' dtype, summed on the host (tests/test_gpu_triple_kernels.py)."""
    out = torch.zeros((n,) + tuple(vals.shape[1:]), dtype=vals.dtype)
    return out.index_add_(0, keys.cpu(), vals.cpu()).to(vals.device)


def bits(x):
    return x.contiguous().view(torch.int32)


class OpCase(object):
    """One spec on `device`: inputs, the float64 reference, the per-triple scales and per-row bounds S_rho, the fp32
    restatement and the checks on the inputs -- computed once and shared by every test of the spec."""

    def __init__(self, spec, device='cpu'):
        self.spec, self.kind, self.dims, self.B, self.tag = spec, spec.kind, spec.dims, spec.B, spec.id
        tabs, params, h, t, r, go = make_inputs(spec)
        self.kinked = 0.0
        if self.kind == 'convkb':
            kink = convkb_kinks(tabs + params, h, t, r)
            self.kinked = float(kink.float().mean())
            assert self.kinked <= 0.03, (self.tag, 'share of the batch inside the ReLU kink band', self.kinked)
            go = torch.where(kink, torch.zeros_like(go), go)
        self.tabs, self.params = [x.to(device) for x in tabs], [x.to(device) for x in params]
        self.h, self.t, self.r, self.go = (x.to(device) for x in (h, t, r, go))
        self.layout = table_layout(self.kind, self.dims)
        self.setup()

    def keys(self, X):
        return torch.cat([self.h, self.t]) if self.layout[X][0] == 'ht' else self.r

    def reference(self, dtype):
        """(scores, [G_X], [layer gradients]) of the restatement in `dtype` under autograd with the gathered rows as
        leaves: G_X is (2B, w) for an entity table (rows of h, then of t) and (B, w) for a relation table."""
        B, kind, dims = self.B, self.kind, self.dims
        a = torch.arange(B, device=self.h.device)
        L = [x[self.keys(X)].to(dtype).requires_grad_(True) for X, x in enumerate(self.tabs)]
        P = [x.detach().to(dtype).clone().requires_grad_(True) for x in self.params]
        f64 = dtype == torch.float64
        if kind in ('rescal', 'hole'):
            s = (triple_sf64(kind, L, dims[0], L[1].shape[1], a, B + a, a) if f64
                 else bilinear_sf(kind, L[0], L[1], dims[0], a, B + a, a))
        elif kind == 'transr':
            s = triple_sf64(kind, L, dims[0], dims[1], a, B + a, a)         # (takes the dtype of its arguments)
        elif kind == 'analogy':
            s = ar.sf64(L, a, B + a, a) if f64 else analogy_sf(L, a, B + a, a)
        else:
            s = cr.sf64(L + P, a, B + a, a) if f64 else convkb_sf(L + P, a, B + a, a)
        assert s.dtype == dtype
        (s * self.go.to(dtype)).sum().backward()
        return (s.detach(), [x.grad if x.grad is not None else torch.zeros_like(x) for x in L], [x.grad for x in P])

    def setup(self):
        tag, B, go = self.tag, self.B, self.go
        self.s64, G64, self.P64 = self.reference(torch.float64)
        s32, G32, P32 = self.reference(torch.float32)
        if self.kind == 'convkb':
            z = torch.logit(self.s64)
            assert float(z.abs().max()) <= 4.0, (tag, 'ConvKB |z| in float64', float(z.abs().max()))
        self.s_tol = TOL * self.s64.abs().clamp_min(1.0)
        err32 = (s32.double() - self.s64).abs()
        self.score32 = float((err32 / self.s_tol).max())
        assert self.score32 <= 0.25, (tag, 'fp32 restatement of the scores: the inputs are wrong', self.score32)
        normd = NORMALISED.get(self.kind, ())
        zero = {X: (self.tabs[X] == 0).all(1) for X in normd}
        uses = torch.zeros(B, dtype=torch.bool, device=go.device)
        for X in normd:
            z = zero[X][self.keys(X)]
            uses |= z[:B] | z[B:]
        ok = (go != 0) & ~uses
        self.rows, self.tri, self.ratio32 = [], [], []
        for X, tab in enumerate(self.tabs):
            keys = self.keys(X)
            rep = keys.shape[0] // B
            n, w = tab.shape
            if w == 0:                      # (ANALOGY without scalar or without complex coordinates)
                self.rows.append(None)
                self.tri.append(None)
                self.ratio32.append(0.0)
                continue
            unit = X in normd and w == 1    # rows of width 1 normalise to +-1: the gradient is exactly zero
            if unit:
                G64[X] = torch.zeros_like(G64[X])
            gmax = G64[X].abs().amax(1)
            ago, okx = go.abs().double().repeat(rep), ok.repeat(rep)
            m = (gmax[okx] / ago[okx]).max() if bool(okx.any()) else gmax.new_zeros(())
            scale = ago * m
            if X in normd:
                scale = torch.where(zero[X][keys], gmax, scale)
            self.tri.append((G64[X], scale))
            self.rows.append((row_sum(n, keys, G64[X]), row_sum(n, keys, scale), row_sum(n, keys, torch.ones_like(scale)) > 0))
            self.ratio32.append(0.0 if unit else max(self.ratio(X, row_sum(n, keys, G32[X])), self.tri_ratio(X, G32[X])))
        assert max(self.ratio32) <= GRAD_TOL / 10, (tag, 'fp32 restatement of the gradients: the inputs are wrong', self.ratio32)
        self.param32 = [self.param_ratio(k, x) for k, x in enumerate(P32)]
        assert max(self.param32 + [0.0]) <= 0.1, (tag, 'fp32 restatement of the layer gradients: the inputs are wrong', self.param32)

    def ratio(self, X, got):
        """max |got - ref| / S_rho over table X (0 / 0 = 0, x / 0 = inf); rows no triple hits must be bit-zero."""
        ref, S, hit = self.rows[X]
        assert got.shape == ref.shape and got.dtype == torch.float32, (self.tag, X)
        assert bool(torch.isfinite(got).all()), (self.tag, 'table', X, 'not finite')
        assert not bool(bits(got[~hit]).any()), (self.tag, 'table', X, 'a row that no triple hits is not bit-zero')
        err = (got.double() - ref).abs().amax(1)
        return float(torch.where(err == 0, torch.zeros_like(err), err / S).max())

    def tri_ratio(self, X, got):
        """The same per TRIPLE: max |row - G[i, X]| / scale_i over the gradient rows (2B or B of them) of table X."""
        ref, scale = self.tri[X]
        assert got.shape == ref.shape and got.dtype == torch.float32, (self.tag, X)
        assert bool(torch.isfinite(got).all()), (self.tag, 'rows of table', X, 'not finite')
        err = (got.double() - ref).abs().amax(1)
        return float(torch.where(err == 0, torch.zeros_like(err), err / scale).max())

    def param_ratio(self, k, got):
        """max |got - ref| / (PARAM_TOL max(1, |ref|max)) of ConvKB's layer gradient k."""
        ref = self.P64[k]
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (self.tag, 'layer gradient', k)
        return float((got.double() - ref).abs().max()) / (PARAM_TOL * max(1.0, float(ref.abs().max())))

    def score_ratio(self, s):
        assert s.shape == self.s64.shape and s.dtype == torch.float32 and bool(torch.isfinite(s).all()), self.tag
        return float(((s.double() - self.s64).abs() / self.s_tol).max())


@pytest.mark.parametrize('spec', SPECS, ids=[s.id for s in SPECS])
def test_inputs_of_every_shape_pass_the_three_conditions(spec):
    """The constructor asserts them; the figures are printed (DESIGN.md section 6 records the largest per kind)."""
    case = OpCase(spec)
    if spec.kind == 'convkb':
        assert spec.dims[0] * spec.dims[1] <= 2112      # (values of v per triple)
    print('operator triples %s (CPU): fp32 restatement score error / bound %.3g, gradient ratio per table %s, layer gradients %s, '
          'zeroed share %.3g' % (case.tag, case.score32, ' '.join('%.3g' % q for q in case.ratio32),
                                 ' '.join('%.3g' % q for q in case.param32) or '-', case.kinked))


def test_the_spec_list_is_the_issues():
    """Every width bucket of every kind, one id per case, and the shapes that reach each code path: lane loops past 64
    and at the 512 edge, TransR's dv chunks 1 and 7 (d_e = 65 / 449), both directions of rows_ld = max(d_e, d_r), ConvKB's
    j stride past 256 and F + 1 > 7 blocks."""
    assert len({s.id for s in SPECS}) == len(SPECS)
    assert {s.dims for s in BUCKET_SPECS if s.kind == 'transr'} >= {(1, 512), (512, 1), (448, 5), (449, 5), (512, 512)}
    assert all(s.B % 4 != 0 for s in SPECS)
    assert all((s.B == 203) == (max(s.dims) <= 129) for s in BUCKET_SPECS)
    assert max(d for s in BUCKET_SPECS if s.kind == 'convkb' for d in s.dims[:1]) == 512
    assert analogy_scale((512, 512)) < analogy_scale((1, 0)) == 0.5
    assert math.isclose(analogy_scale((512, 512)) ** 3 * 1536, 2.0)
