"""The 64 x 64 criterion tile (torchkge_amd/csrc/lp_tile64.h) at every column slice, wave-tile count, staging edge and
chunk split of tests/tile64_table.py, through both criteria that run on it: kge_lp_xent_* and kge_lp_bce_* (run with
-m gpu on an MI355X).

Layer A: forward and backward of both criteria against their float64 forms -- check() of tests/test_gpu_xent.py and
         tests/test_gpu_bce.py as they stand, with their yardstick (tests/xent_ref.py, tests/bce_ref.py on the engine's own
         fp32 scores), comparator (torch's fp32) and bound 4 * (2 * |torch fp32 - float64| + one ulp), at eps 0 and 0.1:
         every K row of the table, the two-slice rows again with three row panels and two chunks, every N row with labels
         and targets on both sides of every chunk boundary.
Layer B: bit equality, BCE at eps = 0.  There y is 0 or 1 and G(i, c) = g_i (sigma(s) - y) depends on nothing outside
         element (i, c), so by the "Order" paragraphs of include/kge_hip_bce.h the call on all N candidates equals what the
         calls on the chunks' candidate slices give: dT rows of a slice are the slice's dT, and -- where every chunk has at
         most MIN_TILES_PER_CHUNK tiles, so that a slice alone is one chunk -- dA is the slices' dA added in ascending
         order.  This pins what the float64 bound cannot see: the tile range of every chunk, the label cursor's start per
         chunk, the [chunk][row][K] indexing of the workspace across both column slices, the ascending order of sum_chunks.
Layer C: bit equality, xent at eps = 0: row_loss = lse - (the pair kernel's score of the target) with the targets walking
         over EVERY (row, candidate) of a three-panel, three-tile problem at the staging rows of the table, and lse /
         row_loss unchanged when the operands' base is 1..3 floats off a 16-byte boundary (16-byte pieces -> scalar loads).

No tolerance of this module's own: every inexact comparison is within() of the two modules above, the rest is equality of
bits.  Shapes come from the constants the headers publish, through tests/tile64_table.py."""
import contextlib
import math
import os
import re

import pytest
import torch

from tests import tile64_table as tt
from tests import test_gpu_bce as tb
from tests import test_gpu_xent as tx
from tests.helpers import carve
from torchkge_amd import _hip_bce, _hip_xent

pytestmark = pytest.mark.gpu

# the table asserts its own buckets when this module is collected (no GPU needed for that)
tt.verify(_hip_xent, _hip_bce)

G = _hip_xent           # the geometry both criteria publish (verify() holds them equal)
RECORD = []             # lines of the parity record (the parity_record fixture writes them out)
WORST = {}              # (criterion, output) -> the largest |fused - f64| / bound seen, and where
EPS = (0.0, 0.1)


@pytest.fixture(scope='module')
def XE():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    _hip_xent.load_library()
    return _hip_xent


@pytest.fixture(scope='module')
def XB():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    _hip_bce.load_library()
    return _hip_bce


@pytest.fixture(scope='module', autouse=True)
def parity_record():
    """After the module: the distances its tests measured go to the file KGE_TILE64_PARITY_OUT names, when it names one
    (profiles/r12/tile64_matrix.txt is one such run)."""
    yield
    path = os.environ.get('KGE_TILE64_PARITY_OUT')
    if path and RECORD:
        with open(path, 'w') as f:
            f.write('max-norm distances to the float64 forms of the engine\'s own fp32 scores '
                    '(tests/test_gpu_tile64_matrix.py)\n')
            f.write('\n'.join(RECORD) + '\n')
            f.write('%d comparisons\n' % len(RECORD))
            for (crit, name), (ratio, tag) in sorted(WORST.items()):
                f.write('worst |fused - f64| / bound of %-4s %-8s %.3g  (%s)\n' % (crit, name, ratio, tag))


@contextlib.contextmanager
def recorded(mod, crit):
    """The within() lines a check() of `mod` appends go to THIS module's record, and leave `mod`'s own as it was."""
    n = len(mod.RECORD)
    worst = dict(getattr(mod, 'WORST', {}))
    try:
        yield
    finally:
        lines = mod.RECORD[n:]
        del mod.RECORD[n:]
        if hasattr(mod, 'WORST'):
            mod.WORST.clear()
            mod.WORST.update(worst)
        for line in lines:
            RECORD.append('%-4s %s' % (crit, line))
            m = re.match(r'(\S+)\s+(.*?)\s+\|fused - f64\| (\S+) .* bound (\S+)', line)
            ratio = float(m.group(3)) / float(m.group(4))       # (the bound holds at least one ulp: never zero)
            if ratio > WORST.get((crit, m.group(1)), (-1.0, ''))[0]:
                WORST[(crit, m.group(1))] = (ratio, m.group(2))


def bits(x):
    return x.contiguous().view(torch.int32)


def _seed(B, N, K):
    return B * 1000 + N + 7 * K[0] + 13 * K[1]


# ---------------------------------------------------------------------------
# labels and targets on both sides of every chunk boundary
# ---------------------------------------------------------------------------
def boundary_sets(B, N, gen):
    """Label sets of B rows: random ones (tests/test_gpu_bce.random_sets), and in front of them one row holding
    {c_j - 1, c_j} for every chunk boundary c_j, one hub row of more than 2 BN labels spread over all chunks, then one row
    {c_j - 1, c_j} per boundary -- as many of these as fit beside at least one random row."""
    cols = tt.chunk_cols(G, N)
    pairs = [[c - 1, c] for c in cols[1:-1]]
    per = -(-(2 * G.BN + 1) // (len(cols) - 1)) + 1
    hub = []
    for c0, c1 in zip(cols, cols[1:]):
        assert c1 - c0 >= per
        hub += [c0 + int(o) for o in torch.randperm(c1 - c0, generator=gen)[:per]]
    hub = sorted(set(hub) | {N - 1})
    assert len(hub) > 2 * G.BN
    special = [sorted(c for p in pairs for c in p), hub] + pairs
    sets = tb.random_sets(B, N, gen)
    n = min(len(special), B - 1)
    sets[:n] = special[:n]
    return sets


def boundary_targets(B, N, t):
    """`t` with its first entries replaced: c_j - 1 and c_j for every chunk boundary, then 0 and N - 1."""
    cols = tt.chunk_cols(G, N)
    first = [c + o for c in cols[1:-1] for o in (-1, 0)] + [0, N - 1]
    n = min(len(first), B)
    t = t.clone()
    t[:n] = torch.tensor(first[:n], dtype=t.dtype, device=t.device)
    return t


def run_xent(XE, B, N, K, tag, boundaries=False):
    A, T, t, w = tx.make(B, N, K[0], K[1], seed=_seed(B, N, K))
    if boundaries:
        t = boundary_targets(B, N, t)
    with recorded(tx, 'xent'):
        for eps in EPS:
            tx.check(XE, A, T, t, w, K[0], K[1], eps, '%s eps=%g' % (tag, eps))


def run_bce(XB, B, N, K, tag, boundaries=False):
    A, T, lab, w = tb.make(B, N, K[0], K[1], seed=_seed(B, N, K))
    if boundaries:
        lab = tb.csr(boundary_sets(B, N, torch.Generator().manual_seed(_seed(B, N, K) + 1)))
    with recorded(tb, 'bce'):
        for eps in EPS:
            tb.check(XB, A, T, lab, w, K[0], K[1], eps, '%s eps=%g' % (tag, eps))


# ---------------------------------------------------------------------------
# Layer A: the K matrix and the N matrix against the float64 forms
# ---------------------------------------------------------------------------
def _k_cases():
    B, N = G.BM + 1, 2 * G.BN + 3
    cases = [(B, N, (K0, K1)) for K0, K1, _, _ in tt.k_table(G)]
    # three row panels, two chunks and two column slices at once
    B3, N2 = 2 * G.BM + 5, G.MIN_TILES_PER_CHUNK * G.BN + 1 + G.BN + 1
    assert tt.chunks(G, N2) == 2 and -(-B3 // G.BM) == 3
    cases += [(B3, N2, kk) for kk in tt.four_slice_rows(G)]
    assert all(tt.slices(G, *kk) == 2 for kk in tt.four_slice_rows(G))
    return cases


def _n_cases():
    cases = []
    for N, T, _, _, _, _ in tt.n_table(G):
        for B in (3, G.BM + 1):
            cases += [(B, N, (8, 0)), (B, N, (5, 0))]
    N129 = tt.n_row(G, G.MIN_TILES_PER_CHUNK * G.MAX_CHUNKS + 1)[0]
    cases.append((G.BM + 1, N129, (G.KSLICE + 8, 8)))       # MAX_CHUNKS workspace panels of two column slices
    return cases


K_CASES, N_CASES = _k_cases(), _n_cases()


def _ids(cases):
    return ['B%d-N%d-K%d+%d' % (b, n, k[0], k[1]) for b, n, k in cases]


@pytest.mark.parametrize('B,N,K', K_CASES, ids=_ids(K_CASES))
def test_xent_at_every_width_of_the_table(XE, B, N, K):
    run_xent(XE, B, N, K, 'B=%d N=%d K=%d+%d' % (B, N, K[0], K[1]))


@pytest.mark.parametrize('B,N,K', K_CASES, ids=_ids(K_CASES))
def test_bce_at_every_width_of_the_table(XB, B, N, K):
    run_bce(XB, B, N, K, 'B=%d N=%d K=%d+%d' % (B, N, K[0], K[1]))


@pytest.mark.parametrize('B,N,K', N_CASES, ids=_ids(N_CASES))
def test_xent_at_every_chunk_split_of_the_table(XE, B, N, K):
    run_xent(XE, B, N, K, 'B=%d N=%d K=%d+%d' % (B, N, K[0], K[1]), boundaries=True)


@pytest.mark.parametrize('B,N,K', N_CASES, ids=_ids(N_CASES))
def test_bce_at_every_chunk_split_of_the_table(XB, B, N, K):
    run_bce(XB, B, N, K, 'B=%d N=%d K=%d+%d' % (B, N, K[0], K[1]), boundaries=True)


# ---------------------------------------------------------------------------
# Layer B: the chunk partition and the chunk-sum order, bit for bit (BCE, eps = 0)
# ---------------------------------------------------------------------------
_M, _C = G.MIN_TILES_PER_CHUNK, G.MAX_CHUNKS
ADDITIVE_T = (3 * _M - 2, 3 * _M - 1, _M * (_C - 1) + 1, _M * _C)       # unequal chunks; MAX_CHUNKS chunks
ALIGNED_T = (_M * _C + 1, _M * _C + 5)                                   # past the cap: dT only
SLICE_KS = ((5, 0), (G.KSLICE + 8, 8))
B_CASES = [(T, K) for T in ADDITIVE_T + ALIGNED_T for K in SLICE_KS]
assert all(tt.n_row(G, T)[4] for T in ADDITIVE_T) and not any(tt.n_row(G, T)[4] for T in ALIGNED_T)


@pytest.mark.parametrize('T,K', B_CASES, ids=['T%d-K%d+%d' % (t, k[0], k[1]) for t, k in B_CASES])
def test_bce_gradients_are_those_of_the_chunks_candidate_slices(XB, T, K):
    """dT[c_j : c_j+1] == dT of the problem on T[c_j : c_j+1] (row views of the same table, every row's labels restricted
    to the slice and shifted by -c_j), and -- where a slice alone is one chunk -- dA == the slices' dA added in ascending
    j with plain fp32 adds.  Labels sit on both sides of every boundary (boundary_sets)."""
    N, _, chunks, _, additive, _ = tt.n_row(G, T)
    B, (K0, K1) = G.BM + 1, K
    A, Tm, _, w = tb.make(B, N, K0, K1, seed=_seed(B, N, K))
    sets = boundary_sets(B, N, torch.Generator().manual_seed(T))
    As, Ts = tb.segs(A, K0, K1), tb.segs(Tm, K0, K1)
    rc, dA, dT = tb.bwd(XB, tb.problem(As, Ts), tb.csr(sets), 0.0, w, dA='new' if additive else None)
    assert rc == 0
    cols = tt.chunk_cols(G, N)
    assert len(cols) == chunks + 1
    acc, bad_t = None, []
    for j, (c0, c1) in enumerate(zip(cols, cols[1:])):
        sub = tb.problem(As, [t[c0:c1] for t in Ts])
        assert sub.N == c1 - c0 and (not additive or XB.chunks(sub.N) == 1)
        lab = tb.csr([[c - c0 for c in s if c0 <= c < c1] for s in sets])
        rc, dAj, dTj = tb.bwd(XB, sub, lab, 0.0, w, dA='new' if additive else None)
        assert rc == 0
        if not all(torch.equal(bits(f[c0:c1]), bits(p)) for f, p in zip(dT, dTj)):
            bad_t.append(j)
        if additive:
            acc = dAj if acc is None else [a + b for a, b in zip(acc, dAj)]
    assert not bad_t, 'dT rows of the chunks %s differ from their slices\' dT' % bad_t
    if additive:
        for seg, (f, s) in enumerate(zip(dA, acc)):
            diff = (bits(f) != bits(s)).nonzero()
            assert diff.numel() == 0, 'dA segment %d differs from the ascending sum of the slices at %d elements, first %s' % (
                seg, diff.shape[0], diff[0].tolist())


# ---------------------------------------------------------------------------
# Layer C: every element of the score tile, bit for bit (xent, eps = 0)
# ---------------------------------------------------------------------------
STAGING_KS = [(K0, K1) for K0, K1, group, _ in tt.k_table(G) if group == tt.STAGING]


@pytest.mark.parametrize('K', STAGING_KS, ids=['K%d+%d' % k for k in STAGING_KS])
def test_xent_target_scores_have_the_pair_kernels_bits_at_every_row_and_column(XE, K):
    """t[i] = (i k + s) mod N with k coprime to N: for every shift s every candidate is some row's target (B >= N), and
    over the shifts every (row, candidate) of the three panels x three tiles is one.  row_loss == lse - pair score, ONE
    fp32 subtraction (the identity of tests/test_gpu_xent.check)."""
    B, N, (K0, K1) = 2 * G.BM + 5, 2 * G.BN + 3, K
    assert B >= N
    A, T, _, w = tx.make(B, N, K0, K1, seed=_seed(B, N, K))
    k = next(k for k in range(G.BN // 2 + 5, N) if math.gcd(k, N) == 1)
    As, Ts = tx.segs(A, K0, K1), tx.segs(T, K0, K1)
    prob = tx.problem(As, Ts)
    i = torch.arange(B, device='cuda')
    wrong = torch.zeros((), dtype=torch.long, device='cuda')
    lse0 = loss0 = None
    for s in range(N):
        t = (i * k + s) % N
        if s == 0:
            assert sorted(set(t.tolist())) == list(range(N))
        rc, lse, loss = tx.fwd(XE, prob, t, 0.0)
        assert rc == 0
        wrong += (bits(loss) != bits(lse - prob.pair_scores(t))).sum()
        if s == 0:
            lse0, loss0 = lse, loss
        else:       # lse does not depend on the targets
            wrong += (bits(lse) != bits(lse0)).sum()
    assert int(wrong) == 0
    # the same operands 1..3 floats off a 16-byte boundary, out of NaN-poisoned padded buffers: scalar loads, the same bits
    t = (i * k) % N
    for off, pad in ((1, 4), (2, 0), (3, 3)):
        Ac, Tc = [carve(x, pad=pad, off=off) for x in As], [carve(x, pad=pad, off=off) for x in Ts]
        assert all(x.data_ptr() % 16 == 4 * off for x in Ac + Tc)
        rc, lse, loss = tx.fwd(XE, tx.problem(Ac, Tc), t, 0.0)
        assert rc == 0
        assert torch.equal(bits(lse), bits(lse0)) and torch.equal(bits(loss), bits(loss0)), (off, pad)
