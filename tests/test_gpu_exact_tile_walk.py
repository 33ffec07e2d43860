"""GPU tests (run with -m gpu on an MI355X) of the exact all-candidates kernels -- lp_gemm_mfma.hip (fp32 MFMA tiles) and
lp_direct.hip (VALU tiles, scalar and packed-FMA) -- where a workgroup walks MANY tiles: the prefetch stream crossing
from one item to the next, the row-panel change inside one block's range, the flush of the 8-bit rank counters, the next
tile's rank-1 scalars, accumulators re-zeroed in the epilogue; and the K tails, wave layouts and operand layouts the
one-tile-per-block shapes of tests/test_gpu_parity.py do not choose.

Everything is compared BIT FOR BIT with the fmaf chains of oracle/kge_oracle.c (orc_lp_gemm_chain, orc_lp_proj_chain,
orc_row_sqnorm_chain, orc_lp_direct_chain): scores with array_equal, counts as integers, no tolerance anywhere.  The
premise of every many-tile case (items per block, a panel boundary inside a range, tiles between two counter flushes,
tiles per block) is asserted through include/kge_hip_plan.h -- the arithmetic the kernels themselves run -- and FAILS,
never skips, when the device's compute-unit count would make the case vacuous.  The launch knobs are environment
variables the library reads at every launch."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from tests.helpers import oracle_clib, fptr

pytestmark = pytest.mark.gpu

i64 = ctypes.c_int64
KNOBS = ('KGE_LP_ROUNDS', 'KGE_LP_WAVES', 'KGE_LP_TARGET_BLOCKS', 'KGE_DIRECT_SCALAR')
ORACLE_THREADS = 8      # the CPU chains run a block of query rows per thread (ctypes releases the GIL)


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def dev(x):
    return torch.as_tensor(x).cuda()


def set_waves(monkeypatch, waves):
    if waves == 8:
        monkeypatch.setenv('KGE_LP_WAVES', '8')     # the 4x2 wave layout; the default (unset) is 2x2


# ---------------------------------------------------------------------------
# the oracle's chains, a block of query rows per thread
# ---------------------------------------------------------------------------
def _by_rows(B, fn):
    step = max(1, -(-B // ORACLE_THREADS))
    spans = [(i, min(i + step, B)) for i in range(0, B, step)]
    if len(spans) == 1:
        fn(*spans[0])
        return
    with ThreadPoolExecutor(len(spans)) as ex:
        list(ex.map(lambda s: fn(*s), spans))


def _c(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.int64)
    return a


def sqnorm_ref(X):
    X = _c(X)
    out = np.empty(X.shape[0], dtype=np.float32)
    oracle_clib().orc_row_sqnorm_chain(fptr(X), i64(X.shape[1]), i64(X.shape[0]), i64(X.shape[1]), fptr(out))
    return out


def gemm_ref(A0, T0, A1=None, T1=None, qn=None, en=None):
    """orc_lp_gemm_chain: DOT (one or two segments), or L2_EXPAND when qn / en are given."""
    lib = oracle_clib()
    A0, T0 = _c(A0), _c(T0)
    B, K0 = A0.shape
    N = T0.shape[0]
    K1 = 0 if A1 is None else A1.shape[1]
    if K1:
        A1, T1 = _c(A1), _c(T1)
    out = np.empty((B, N), dtype=np.float32)

    def part(i0, i1):
        lib.orc_lp_gemm_chain(fptr(A0[i0:i1]), i64(K0), fptr(T0), i64(K0), i64(K0),
                              fptr(A1[i0:i1]) if K1 else None, i64(K1), fptr(T1) if K1 else None, i64(K1), i64(K1),
                              i64(i1 - i0), i64(N), 1 if qn is not None else 0,
                              fptr(qn[i0:i1]) if qn is not None else None, fptr(en) if qn is not None else None,
                              fptr(out[i0:i1]))
    _by_rows(B, part)
    return out


def proj_ref(mode_name, A, T, qn, en, X, r_idx, yc, pz):
    lib = oracle_clib()
    A, T, X, r_idx, yc, pz = _c(A), _c(T), _c(X), _c(r_idx), _c(yc), _c(pz)
    B, K = A.shape
    N = T.shape[0]
    out = np.empty((B, N), dtype=np.float32)

    def part(i0, i1):
        lib.orc_lp_proj_chain(ctypes.c_int(4 if mode_name == 'projh' else 5), fptr(A[i0:i1]), i64(K), fptr(T), i64(K),
                              i64(K), i64(i1 - i0), i64(N), fptr(qn[i0:i1]), fptr(en), fptr(X), i64(X.shape[1]),
                              fptr(r_idx[i0:i1]), fptr(yc), fptr(pz[i0:i1]), fptr(out[i0:i1]))
    _by_rows(B, part)
    return out


def direct_ref(Q, T, p, W=None, scal=None, ridx=None):
    """orc_lp_direct_chain; scal (N, R) with ridx, or (N,) (scal_ld == 1) without."""
    lib = oracle_clib()
    Q, T = _c(Q), _c(T)
    B, K = Q.shape
    N = T.shape[0]
    if W is not None:
        W, scal = _c(W), _c(scal)
        scal_ld = 1 if scal.ndim == 1 else scal.shape[1]
        assert (ridx is not None) == (scal_ld > 1)
        if ridx is not None:
            ridx = _c(ridx)
    out = np.empty((B, N), dtype=np.float32)

    def part(i0, i1):
        lib.orc_lp_direct_chain(fptr(Q[i0:i1]), i64(K), fptr(T), i64(K), i64(K),
                                fptr(W[i0:i1]) if W is not None else None, i64(K),
                                fptr(scal) if W is not None else None, i64(scal_ld if W is not None else 0),
                                fptr(ridx[i0:i1]) if ridx is not None else None, i64(i1 - i0), i64(N), p,
                                fptr(out[i0:i1]))
    _by_rows(B, part)
    return out


# ---------------------------------------------------------------------------
# problems: host operands, their oracle matrix, the device descriptor
# ---------------------------------------------------------------------------
MFMA_FORMS = ('dot', 'dot2', 'expand', 'projh', 'projd')
N_REL = 5


def mfma_operands(form, B, N, K0, K1, seed):
    """Host operands of one MFMA-mode problem and its oracle matrix 'ref'."""
    g = torch.Generator().manual_seed(seed)
    o = {'form': form}
    if form in ('projh', 'projd'):
        o['A0'] = (torch.randn(B, K0, generator=g) * 0.3).numpy()
        o['T0'] = (torch.randn(N, K0, generator=g) * 0.3).numpy()
        o['X'] = (torch.randn(N_REL, N, generator=g) * 0.2).numpy()
        o['yc'] = (torch.randn(N, generator=g) * 0.2).numpy()
        o['pz'] = (torch.randn(B, 2, generator=g) * 0.5).numpy()
        o['r_idx'] = torch.randint(0, N_REL, (B,), generator=g).numpy()
    else:
        o['A0'] = (torch.rand(B, K0, generator=g) * 2 - 1).numpy()
        o['T0'] = (torch.rand(N, K0, generator=g) * 2 - 1).numpy()
    if form == 'dot2':
        o['A1'] = (torch.rand(B, K1, generator=g) * 2 - 1).numpy()
        o['T1'] = (torch.rand(N, K1, generator=g) * 2 - 1).numpy()
    if form != 'dot' and form != 'dot2':
        o['qn'], o['en'] = sqnorm_ref(o['A0']), sqnorm_ref(o['T0'])
    if form == 'dot':
        o['ref'] = gemm_ref(o['A0'], o['T0'])
    elif form == 'dot2':
        o['ref'] = gemm_ref(o['A0'], o['T0'], o['A1'], o['T1'])
    elif form == 'expand':
        o['ref'] = gemm_ref(o['A0'], o['T0'], qn=o['qn'], en=o['en'])
    else:
        o['ref'] = proj_ref(form, o['A0'], o['T0'], o['qn'], o['en'], o['X'], o['r_idx'], o['yc'], o['pz'])
    return o


def mfma_problem(hip, o, over=None):
    """The device problem of mfma_operands(); `over`: device tensors to use instead of fresh copies (layout cases)."""
    form = o['form']
    t = {k: dev(o[k]) for k in ('A0', 'T0', 'A1', 'T1', 'qn', 'en', 'X', 'yc', 'pz', 'r_idx') if k in o}
    t.update(over or {})
    if 'qn' in t:       # the device's own norms are the oracle's chain, bit for bit
        assert torch.equal(hip.row_sqnorm(t['A0']), t['qn']) and torch.equal(hip.row_sqnorm(t['T0']), t['en'])
    if form == 'dot':
        return hip.LpProblem(hip.LP_DOT, t['A0'], t['T0'])
    if form == 'dot2':
        return hip.LpProblem(hip.LP_DOT, t['A0'], t['T0'], A1=t['A1'], T1=t['T1'])
    if form == 'expand':
        return hip.LpProblem(hip.LP_L2_EXPAND, t['A0'], t['T0'], qn=t['qn'], en=t['en'])
    return hip.LpProblem(hip.LP_L2_PROJH if form == 'projh' else hip.LP_L2_PROJD, t['A0'], t['T0'], qn=t['qn'], en=t['en'],
                         Wq=t['pz'], scal=t['X'], r_idx=t['r_idx'], yc=t['yc'] if form == 'projd' else None)


def direct_operands(p, B, N, K, axpy, seed):
    """Host operands of one L1 / L2 broadcast-subtract problem and its oracle matrix; axpy: None, 'ridx' (scal (N, R)
    with r_idx) or 'one' (scal (N,), scal_ld == 1).  The rank-1 scalars differ from column to column."""
    g = torch.Generator().manual_seed(seed)
    o = {'p': p, 'axpy': axpy}
    o['A0'] = (torch.rand(B, K, generator=g) * 2 - 1).numpy()
    o['T0'] = (torch.rand(N, K, generator=g) * 2 - 1).numpy()
    if axpy:
        o['Wq'] = (torch.rand(B, K, generator=g) - 0.5).numpy()
        o['scal'] = (torch.rand(N, N_REL, generator=g) - 0.5).numpy() if axpy == 'ridx' else (torch.rand(N, generator=g) - 0.5).numpy()
        if axpy == 'ridx':
            o['r_idx'] = torch.randint(0, N_REL, (B,), generator=g).numpy()
    o['ref'] = direct_ref(o['A0'], o['T0'], p, o.get('Wq'), o.get('scal'), o.get('r_idx'))
    return o


def direct_problem(hip, o, over=None):
    t = {k: dev(o[k]) for k in ('A0', 'T0', 'Wq', 'scal', 'r_idx') if k in o}
    t.update(over or {})
    return hip.LpProblem(hip.LP_L1_DIRECT if o['p'] == 1 else hip.LP_L2_DIRECT, t['A0'], t['T0'], Wq=t.get('Wq'),
                         scal=t.get('scal'), r_idx=t.get('r_idx'))


def check_scores_pairs_counts(prob, ref, seed, tag, ci=None, scores=True):
    """The three checks: scores() == oracle matrix; pair_scores() on drawn candidates == oracle entries; count_ge() ==
    (ref >= ref[true]) summed.  `ci`: the candidates to draw (default: uniform)."""
    B, N = ref.shape
    if scores:
        assert np.array_equal(prob.scores().cpu().numpy(), ref), tag
    if ci is None:
        ci = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(seed)).numpy()
    want = ref[np.arange(B), ci]
    st = prob.pair_scores(dev(ci))
    assert np.array_equal(st.cpu().numpy(), want), tag
    assert np.array_equal(prob.count_ge(st).cpu().numpy(), (ref >= want[:, None]).sum(1)), tag


# ---------------------------------------------------------------------------
# (a) + (f)  MFMA kernel, many items per block, a row-panel change inside a block's range
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def walk_shape():
    """(B, N, plan) taken from the launcher's own split on THIS device: three row panels (the last partial), a partial
    last candidate tile, and the smallest N at which every block holds >= 3 items and some block's range has a panel
    boundary strictly inside."""
    from torchkge_amd import _hip_plan
    BM, BN = _hip_plan.GEMM_BM, _hip_plan.GEMM_BN
    B = 2 * BM + 37
    probe = _hip_plan.gemm_plan(B, 1 << 24)                 # the grid when items abound: 2 blocks per compute unit
    ct0 = -(-3 * probe.grid // probe.row_panels)
    for ct in range(ct0, ct0 + 64):
        N = ct * BN - 45
        plan = _hip_plan.gemm_plan(B, N)
        if walk_premise(plan)[0] >= 3 and walk_premise(plan)[1] >= 1:
            return B, N, plan
    raise AssertionError('no N near %d tiles gives every block 3 items and one of them a panel change' % ct0)


def walk_premise(plan):
    """(fewest items of a block, blocks with a panel boundary strictly inside their range)."""
    ct = plan.col_tiles
    fewest = min(e - b for _, b, e in plan.blocks)
    inside = sum(1 for _, b, e in plan.blocks if any(b < p * ct < e for p in range(1, plan.row_panels)))
    return fewest, inside


@functools.lru_cache(maxsize=1)
def walk_case(form, K):
    B, N, _ = walk_shape()
    o = mfma_operands(form, B, N, K, K + 8, seed=1000 + K)
    # each query its own threshold, the median of its row: about half of the row counts, and a stale panel vector --
    # another query's median -- changes the count
    o['ci'] = np.argpartition(o['ref'], N // 2, axis=1)[:, N // 2]
    return o


@pytest.mark.parametrize('waves', [4, 8])
@pytest.mark.parametrize('K', [44, 21])         # 44: a 2-block tail on float4 loads; 21: K % 4 != 0, a 3-block tail
@pytest.mark.parametrize('form', MFMA_FORMS)    # dot2: (K0, K1) = (K, K + 8) -- segments of different widths and tails
def test_mfma_many_items_per_block_bit_exact_vs_chain(hip, monkeypatch, form, K, waves):
    """Every block of the launcher's grid walks >= 3 (row panel, tile) items and at least one of them changes its row
    panel on the way (flush_counts + load_panel: new s_true, qn, PROJ scalars): scores (write mode) and counts (count
    mode) against the oracle matrix, on both wave layouts."""
    from torchkge_amd import _hip_plan
    B, N, plan = walk_shape()
    fewest, inside = walk_premise(plan)
    assert plan.row_panels == 3 and B % _hip_plan.GEMM_BM and N % _hip_plan.GEMM_BN
    assert fewest >= 3 and inside >= 1, (fewest, inside)
    set_waves(monkeypatch, waves)
    assert _hip_plan.gemm_plan(B, N).blocks == plan.blocks         # the layout does not change the split
    o = walk_case(form, K)
    prob = mfma_problem(hip, o)
    check_scores_pairs_counts(prob, o['ref'], 0, (form, K, waves, B, N), ci=o['ci'])
    cnt = (o['ref'] >= o['ref'][np.arange(B), o['ci']][:, None]).sum(1)
    assert cnt.min() > N // 4 and cnt.max() < 3 * N // 4 and len(set(o['ref'][np.arange(B), o['ci']].tolist())) > B // 2


# ---------------------------------------------------------------------------
# (b)  the 8-bit counter flush inside one row panel
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def flush_shape():
    """(N, plan): one row panel and the smallest candidate count at which some block of the launcher's grid walks two
    tiles more than the flush interval."""
    from torchkge_amd import _hip_plan
    interval = _hip_plan.gemm_flush_interval()
    slots = _hip_plan.gemm_plan(4, 1 << 34).grid
    N = (interval + 2) * slots * _hip_plan.GEMM_BN - 77
    return N, _hip_plan.gemm_plan(4, N)


@functools.lru_cache(maxsize=1)
def flush_case(form):
    N, _ = flush_shape()
    o = mfma_operands(form, 4, N, 4, 0, seed=77)
    ref = o['ref']
    g = torch.Generator().manual_seed(5)
    # row 0: -inf (every candidate counts: each lane's counter gains its full share of every tile); row 1: the largest
    # score of its row (only its ties count); rows 2, 3: ordinary thresholds
    o['st'] = np.array([-np.inf, ref[1].max(), ref[2, int(torch.randint(0, N, (1,), generator=g))],
                        ref[3, int(torch.randint(0, N, (1,), generator=g))]], dtype=np.float32)
    o['want'] = (ref >= o['st'][:, None]).sum(1)
    return o


@pytest.mark.parametrize('waves', [4, 8])
@pytest.mark.parametrize('form', ['dot', 'expand'])
def test_mfma_counter_flush_inside_one_panel(hip, monkeypatch, form, waves):
    """One row panel, so many candidates that some block walks two tiles more than kge_lp_gemm_flush_interval() of it:
    a counter byte that is not flushed in time spills into its neighbour's row (count mode only)."""
    from torchkge_amd import _hip_plan
    set_waves(monkeypatch, waves)
    N, plan = flush_shape()
    interval = _hip_plan.gemm_flush_interval()
    assert plan.row_panels == 1 and plan.blocks == _hip_plan.gemm_plan(4, N).blocks
    assert max(e - b for _, b, e in plan.blocks) >= interval + 2, interval
    o = flush_case(form)
    assert o['want'][0] == N and 1 <= o['want'][1] < 100 and all(100 < int(w) < N for w in o['want'][2:])
    prob = mfma_problem(hip, o)
    ci = torch.randint(0, N, (4,), generator=torch.Generator().manual_seed(9)).numpy()
    assert np.array_equal(prob.pair_scores(dev(ci)).cpu().numpy(), o['ref'][np.arange(4), ci])
    got = prob.count_ge(dev(o['st'])).cpu().numpy()
    assert np.array_equal(got, o['want']), (form, waves, got, o['want'])


# ---------------------------------------------------------------------------
# (c) + (f)  K tails at one-tile-per-block shapes
# ---------------------------------------------------------------------------
MFMA_K = [1, 8, 9, 16, 17, 24, 25, 31, 32, 33, 40, 41, 48, 57, 64, 65, 100]
# two segments whose tails differ; 'lt': K1 < K0 (among them K1 < 8), 'gt': K1 > K0; float4 and scalar loads
MFMA_K_PAIRS = [(48, 4, 'lt'), (24, 8, 'lt'), (48, 5, 'lt'), (33, 16, 'lt'), (17, 3, 'lt'),
                (16, 24, 'gt'), (24, 100, 'gt'), (9, 40, 'gt'), (17, 57, 'gt'), (64, 65, 'gt')]
DIRECT_K = [1, 3, 4, 5, 8, 12, 20, 31, 32, 33, 36, 60, 64, 68]


def tail_blocks(K):
    """8-blocks of the last BK = 32 step of a K-wide segment (4: a full step)."""
    return -(-(K % 32 or 32) // 8)


def test_the_k_lists_reach_every_tail_branch_on_both_load_paths():
    for blocks in (1, 2, 3, 4):
        for vec4 in (True, False):
            assert any(tail_blocks(K) == blocks and (K % 4 == 0) == vec4 for K in MFMA_K), (blocks, vec4)
    assert all(tail_blocks(a) != tail_blocks(b) and a != b for a, b, _ in MFMA_K_PAIRS)
    assert any(b < 8 for _, b, _ in MFMA_K_PAIRS) and any(b > a for a, b, _ in MFMA_K_PAIRS)
    assert any(K % 4 == 0 for K in DIRECT_K) and any(K % 4 for K in DIRECT_K) and any(K > 64 for K in DIRECT_K)


@pytest.mark.parametrize('waves', [4, 8])
@pytest.mark.parametrize('K', MFMA_K)
def test_mfma_k_tail_matrix_bit_exact_vs_chain(hip, monkeypatch, K, waves):
    set_waves(monkeypatch, waves)
    for form in ('dot', 'expand', 'projh', 'projd'):
        o = mfma_operands(form, 70, 300, K, 0, seed=K)
        check_scores_pairs_counts(mfma_problem(hip, o), o['ref'], K, (form, K, waves))


@pytest.mark.parametrize('waves', [4, 8])
@pytest.mark.parametrize('K0,K1,order', MFMA_K_PAIRS, ids=['%d-%d-%s' % p for p in MFMA_K_PAIRS])
def test_mfma_two_segments_of_different_width_bit_exact_vs_chain(hip, monkeypatch, K0, K1, order, waves):
    set_waves(monkeypatch, waves)
    o = mfma_operands('dot2', 70, 300, K0, K1, seed=K0 * 101 + K1)
    check_scores_pairs_counts(mfma_problem(hip, o), o['ref'], K0, (K0, K1, waves))


@pytest.mark.parametrize('K', DIRECT_K)
def test_direct_k_tail_matrix_bit_exact_vs_chain(hip, monkeypatch, K):
    """L1, L2 (packed-FMA kernel when K % 4 == 0, scalar loads otherwise) and, for K % 4 == 0, L2 on the VEC4 scalar
    kernel (KGE_DIRECT_SCALAR=1: nothing else reaches it); without the rank-1 term, with it through r_idx
    (scal_ld > 1), and with scal_ld == 1."""
    for axpy in (None, 'ridx', 'one'):
        for p in (1, 2):
            o = direct_operands(p, 70, 300, K, axpy, seed=K * 7 + p)
            prob = direct_problem(hip, o)
            check_scores_pairs_counts(prob, o['ref'], K, (K, p, axpy))
            if p == 2 and K % 4 == 0:
                monkeypatch.setenv('KGE_DIRECT_SCALAR', '1')
                check_scores_pairs_counts(prob, o['ref'], K, (K, p, axpy, 'scalar kernel'))
                monkeypatch.delenv('KGE_DIRECT_SCALAR')


# ---------------------------------------------------------------------------
# (d)  the float4 paths fall back per OPERAND: one leading dimension or one base address at a time
# ---------------------------------------------------------------------------
def relayout(x, how):
    """x's values in a view whose leading dimension is no multiple of 4 ('ld') or whose base lies 4 bytes past a 16-byte
    boundary ('base': column offset 1 of a wider buffer); the rest of the buffer is NaN."""
    rows, K = x.shape
    assert K % 4 == 0
    if how == 'ld':
        v = torch.full((rows, K + 1), float('nan'), device=x.device)[:, :K]
        assert v.stride(0) % 4 != 0 and v.data_ptr() % 16 == 0
    else:
        v = torch.full((rows, K + 8), float('nan'), device=x.device)[:, 1:K + 1]
        assert v.stride(0) % 4 == 0 and v.data_ptr() % 16 == 4
    v.copy_(x)
    return v


@pytest.mark.parametrize('how', ['ld', 'base'])
@pytest.mark.parametrize('operand', ['A0', 'T0', 'A1', 'T1'])
def test_mfma_float4_fallback_per_operand(hip, operand, how):
    o = mfma_operands('dot2', 70, 300, 40, 24, seed=3)
    aligned = mfma_problem(hip, o)
    S = aligned.scores()
    assert np.array_equal(S.cpu().numpy(), o['ref'])
    prob = mfma_problem(hip, o, over={operand: relayout(dev(o[operand]), how)})
    assert torch.equal(prob.scores(), S)
    check_scores_pairs_counts(prob, o['ref'], 1, (operand, how))


@pytest.mark.parametrize('how', ['ld', 'base'])
@pytest.mark.parametrize('operand', ['A0', 'T0', 'Wq'])
@pytest.mark.parametrize('p', [1, 2])
def test_direct_float4_fallback_per_operand(hip, p, operand, how):
    o = direct_operands(p, 70, 300, 36, 'ridx', seed=4)
    aligned = direct_problem(hip, o)
    S = aligned.scores()
    assert np.array_equal(S.cpu().numpy(), o['ref'])
    prob = direct_problem(hip, o, over={operand: relayout(dev(o[operand]), how)})
    assert torch.equal(prob.scores(), S)
    check_scores_pairs_counts(prob, o['ref'], 1, (p, operand, how))


# ---------------------------------------------------------------------------
# (e)  VALU kernels, one block walks the whole candidate range
# ---------------------------------------------------------------------------
def force_one_block_per_panel(monkeypatch, B, N, axpy):
    from torchkge_amd import _hip_plan
    monkeypatch.setenv('KGE_LP_TARGET_BLOCKS', '1')
    plan = _hip_plan.direct_plan(B, N, axpy)
    assert plan.tiles_per_block == plan.col_tiles > 4 and plan.grid == plan.row_panels, plan[:4]
    assert N % _hip_plan.DIRECT_BN != 0                                     # a partial last tile
    return plan


@pytest.mark.parametrize('axpy', [None, 'ridx'])
@pytest.mark.parametrize('kernel', ['l1', 'l2_packed', 'l2_scalar'])
@pytest.mark.parametrize('B', [70, 130])
def test_direct_many_tiles_per_block_bit_exact_vs_chain(hip, monkeypatch, B, kernel, axpy):
    N, K = 1100, 36
    assert N % 8 == 4
    o = direct_operands(1 if kernel == 'l1' else 2, B, N, K, axpy, seed=B + len(kernel))
    prob = direct_problem(hip, o)
    force_one_block_per_panel(monkeypatch, B, N, axpy is not None)
    if kernel == 'l2_scalar':
        monkeypatch.setenv('KGE_DIRECT_SCALAR', '1')
    check_scores_pairs_counts(prob, o['ref'], B, (B, kernel, axpy))


@pytest.mark.parametrize('mode_name', ['LP_TORUS_L1', 'LP_TORUS_L2', 'LP_TORUS_EL2'])
def test_torus_many_tiles_per_block_equals_the_default_launch(hip, monkeypatch, mode_name):
    """The torus modes have no CPU chain: this is GPU against GPU -- the launch forced to one block per row panel must
    give the bits of the default launch (one tile per block) and of pair_scores()."""
    from torchkge_amd import _hip_plan
    B, N, K = 130, 1100, 36
    g = torch.Generator().manual_seed(11)
    Q, T = torch.rand(B, K, generator=g).cuda(), torch.rand(N, K, generator=g).cuda()
    ci = torch.randint(0, N, (B,), generator=g).cuda()
    prob = hip.LpProblem(getattr(hip, mode_name), Q, T)
    assert _hip_plan.direct_plan(B, N).tiles_per_block == 1
    S0 = prob.scores()
    st = prob.pair_scores(ci)
    c0 = prob.count_ge(st)
    force_one_block_per_panel(monkeypatch, B, N, False)
    S1, c1 = prob.scores(), prob.count_ge(st)
    assert torch.equal(S1, S0) and torch.equal(c1, c0)
    assert torch.equal(st, S1[torch.arange(B, device='cuda'), ci])
    assert torch.equal(c1.long(), (S1 >= st.view(-1, 1)).sum(1)) and int(c1.min()) >= 1
    assert float(S1.std()) > 0


# ---------------------------------------------------------------------------
# (g)  counts over query COLUMNS (packed-FMA kernel): one and four threshold sets per row
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('forced', [False, True])
def test_count_ge_cols_many_tiles_per_block_vs_chain(hip, monkeypatch, forced):
    from tests.helpers import raw
    lib = hip.load_library()
    n_single, n_multi, N, K, GS = 150, 50, 1100, 36, 4
    n_cols = n_single + n_multi
    assert GS == hip.split_group_sets()
    g = torch.Generator().manual_seed(21)
    o = direct_operands(2, n_cols, N, K, None, seed=21)         # row i of A0: the query row of some column
    ref = o['ref']
    rep = torch.randperm(n_cols, generator=g)                   # column r is scored with query row rep[r]
    # queries: one per single column (a few columns carry none), 1..4 per grouped column; query ids are shuffled so
    # that raw_count is indexed by QUERY, not by column
    slots = [(r, 0) for r in range(n_single) if r % 17 != 5]
    n_members = torch.randint(1, GS + 1, (n_multi,), generator=g).tolist()
    n_members[0], n_members[1] = 1, GS
    for m, k in enumerate(n_members):
        for gs in sorted(torch.randperm(GS, generator=g)[:k].tolist()):
            slots.append((n_single + m, gs))
    nq = len(slots)
    qid = torch.randperm(nq, generator=g).tolist()
    col_q = torch.full((n_single,), -1, dtype=torch.int32)
    members = torch.full((n_multi, GS), -1, dtype=torch.int32)
    true = torch.randint(0, N, (nq,), generator=g).numpy()
    st = np.empty(nq, dtype=np.float32)
    want = np.zeros(nq, dtype=np.int64)
    for (r, gs), q in zip(slots, qid):
        if r < n_single:
            col_q[r] = q
        else:
            members[r - n_single, gs] = q
        row = ref[int(rep[r])]
        st[q] = row[true[q]]
        want[q] = (row >= st[q]).sum()
    assert int((members < 0).sum()) > 0 and int((col_q < 0).sum()) > 0 and int((members >= 0).sum(1).max()) == GS
    prob = direct_problem(hip, o)
    if forced:
        force_one_block_per_panel(monkeypatch, n_single, N, False)
        force_one_block_per_panel(monkeypatch, n_multi, N, False)
    cnt = torch.zeros(nq, dtype=torch.int32, device='cuda')
    d_st, d_rep, d_col, d_mem = dev(st), rep.cuda(), col_q.cuda(), members.cuda().contiguous()
    rc = raw(lib, 'kge_lp_count_ge_cols', prob.desc, d_st, cnt, d_rep, d_col, n_single, d_mem, n_multi)
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(cnt.cpu().numpy(), want), forced
