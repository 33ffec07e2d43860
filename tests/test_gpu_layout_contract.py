"""The C ABI's LAYOUT contract on the MI355X: leading dimensions, base offsets, poisoned pads, guarded outputs.

Almost every entry point of include/kge_hip.h takes a pointer AND a leading dimension, and almost every kernel behind
them has two bodies chosen by a host-side predicate `K % 4 == 0 && ld % 4 == 0 && 16-byte aligned base` (vector /
staged / packed-FMA body, else the scalar one).  The other GPU modules hand over fresh contiguous torch tensors (256-byte
aligned, ld == K); here every operand is a view CARVED out of one larger buffer (tests/helpers.py: carve, guarded_out):

  * row stride K + pad, pad in {0, 1, 3, 4, 8}; base `off` in {0, 1, 2, 3} floats past a 16-byte boundary; applied to ONE
    operand at a time (a predicate that forgets an operand only shows when the others are aligned) and to all at once;
  * everything around the view -- the pad of every row and >= 256 rows / elements in front and behind -- holds POISON
    (NaN for arithmetic inputs, additionally +inf / -inf for score matrices that are ranked), so a kernel that
    over-reads fetches poison from inside a live allocation and fails BY VALUE: nothing here is arranged to fault;
  * every output lies in a buffer pre-filled with a sentinel bit pattern that must survive outside the live window.

Per case, in this order: (a) return code 0, (b) equality with the CPU reference on the PACKED data -- bit-exact where
the header states a chain / integer contract (oracle/kge_oracle.c), the existing tolerance of that entry point's test
where it states none --, (c) bit equality with the same call on packed, aligned copies, (d) no poison in the output,
(e) guards intact.  Calls go through ctypes with explicit leading dimensions (helpers.raw): the tensor-level wrappers
would copy a strided view.

Groups: A row primitives; B all-candidates scoring (every kge_lp_desc mode, the pair / count / filter forms, the
pointer-advancing chunk and row-block helpers); C operand builders of the prefilters (bytes equal to those built from the
packed copy; prefilter + recheck counts with a carved exact-score descriptor); D fused entry points that REFUSE
unaligned input (the documented code comes back, nothing was launched, the separate kernels and the Python wrappers give
the fused path's bits); E fused gather + normalise + score, its backward and the gradient reductions, the kge_lp_prep
family (contiguous tables: the layout axis is the base offset, crossed with d % 4); F query transforms (every ld padded);
G rank / filter / top-k on a materialised matrix.

LAYOUT_TABLE holds every exported symbol that no test of this module calls, with the reason: it takes no strided or
alignment-sensitive argument, or it is packed by contract.  A host test (tests/test_oracle_golden.py) checks that every
prototype of the header is called here (raw(), or DRIVEN_THROUGH_LPPROBLEM) or listed with one of those reasons.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import kge_oracle as orc
from tests.helpers import oracle_clib, fptr, carve, guarded_out, assert_guard_intact, raw
from tests.test_gpu_rescal_hole import sf64 as bilinear_sf64, queries64
from tests.test_gpu_toruse import diss64
from tests.test_transr_host import scoring64 as transr_sf64

pytestmark = pytest.mark.gpu

TOL = 1e-5      # the suite's tolerance on scores (tests/test_gpu_parity.py, tests/test_gpu_toruse.py)
NAN, INF = float('nan'), float('inf')
i64 = ctypes.c_int64
KGE_EINVAL, KGE_EUNSUPPORTED = -1, -3

_NO_LAYOUT = 'no strided or alignment-sensitive argument (sizes, integer vectors or opaque workspaces only)'
_PACKED = 'packed by contract (no leading dimension) and no vector-path predicate on its pointers'
REASONS = (_NO_LAYOUT, _PACKED)         # the only reasons the table may give (a host test holds every entry to them)
# Entry points that read a kge_lp_desc plus opaque operands built by other entry points: driven with a CARVED descriptor
# through its Python owner (LpProblem.count_ge), not through raw() -- name -> the test of this module that does
DRIVEN_THROUGH_LPPROBLEM = {
    'kge_lp_split_count': 'test_prefilter_counts_with_a_carved_exact_score_descriptor',
    'kge_lp_split_recheck': 'test_prefilter_counts_with_a_carved_exact_score_descriptor',
    'kge_lp_sad_count': 'test_prefilter_counts_with_a_carved_exact_score_descriptor',
    'kge_lp_sad_recheck': 'test_prefilter_counts_with_a_carved_exact_score_descriptor',
}
LAYOUT_TABLE = {
    # --- nothing to lay out
    'kge_abi_version': _NO_LAYOUT, 'kge_build_arch': _NO_LAYOUT, 'kge_mfma_f16_selftest': _NO_LAYOUT,
    'kge_corrupt_ws_elems': _NO_LAYOUT, 'kge_corrupt_scatter': _NO_LAYOUT, 'kge_key_hist': _NO_LAYOUT,
    'kge_key_scatter': _NO_LAYOUT, 'kge_key_sort': _NO_LAYOUT, 'kge_key_sort_ws_bytes': _NO_LAYOUT,
    'kge_filter_lookup': _NO_LAYOUT, 'kge_filter_lookup_both': _NO_LAYOUT, 'kge_i64_max3': _NO_LAYOUT,
    'kge_filter_index_ws_bytes': _NO_LAYOUT, 'kge_filter_index_build': _NO_LAYOUT, 'kge_filter_plan_ws_bytes': _NO_LAYOUT,
    'kge_filter_plan_build': _NO_LAYOUT, 'kge_column_plan_ws_bytes': _NO_LAYOUT, 'kge_column_plan_build': _NO_LAYOUT,
    'kge_column_plan_emit': _NO_LAYOUT, 'kge_lp_filter_sub_ws_bytes': _NO_LAYOUT, 'kge_lp_split_group_sets': _NO_LAYOUT,
    'kge_lp_split_units': _NO_LAYOUT, 'kge_lp_split_rows_padded': _NO_LAYOUT, 'kge_lp_hi_units': _NO_LAYOUT,
    'kge_lp_hi_stream_supported': _NO_LAYOUT, 'kge_lp_table_prep_blocks': _NO_LAYOUT,
    'kge_lp_dot_table_prep_blocks': _NO_LAYOUT, 'kge_lp_split_regions': _NO_LAYOUT,
    'kge_lp_split_regions_supported': _NO_LAYOUT, 'kge_lp_sad_cols_padded': _NO_LAYOUT,
    'kge_host_device_pointer': _NO_LAYOUT, 'kge_copy_i64_indirect': _NO_LAYOUT,
    'kge_rank_finalize': _PACKED,
    'kge_lp_split_prefix_max': _PACKED + ' (reads the cell sums kge_lp_split_rows wrote)',
}


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip
    _hip.load_library()
    return _hip


# ---------------------------------------------------------------------------
# the layout matrix
# ---------------------------------------------------------------------------
ALL_AT_ONCE = [(0, 0), (1, 0), (3, 0), (4, 0), (8, 0), (0, 1), (0, 2), (0, 3), (1, 1), (3, 2), (4, 3), (8, 1), (4, 2)]
ONE_AT_A_TIME = [(1, 0), (4, 0), (0, 1), (0, 3)]
FEW = [(0, 0), (3, 1), (4, 2), (8, 0), (0, 3)]          # the layouts every shape of the long shape lists sees
OUT_PAD = {0: 0, 1: 1, 3: 5, 4: 4, 8: 5}               # ldo in {N, N + 1, N + 4, N + 5}
INNER = [1, 3, 4, 8, 17, 64, 200, 203, 512]
# (rows / queries, candidates, K): both sides of the kernels' tiles -- 16 / 32 / 64 / 128 / 256 rows (the staged row
# kernels, the MFMA panels of lp_gemm_mfma.hip, the 256-row split panel), 192 / 256 candidates -- and every inner dimension
SHAPES = [(1, 1, 1), (31, 191, 3), (32, 192, 4), (33, 193, 8), (63, 255, 17), (64, 256, 64), (65, 257, 200), (127, 1, 203),
          (128, 192, 512), (129, 257, 4), (255, 193, 8), (256, 256, 17), (257, 255, 64), (1, 257, 200), (15, 17, 48)]
SMALL = [(33, 193, 17), (65, 257, 64)]                  # the shapes that see EVERY layout


def layouts(operands, full=True):
    """Curated list of {operand: (pad, off)}: every operand at once, then one operand at a time with the rest packed and
    aligned.  'out' pads are mapped to the ldo values of the issue, 'vec' (all 1-D operands) only has an offset."""
    out = []
    for pad, off in (ALL_AT_ONCE if full else FEW):
        lay = {o: (pad, off) for o in operands}
        if 'out' in lay:
            lay['out'] = (OUT_PAD[pad], off)
        out.append(lay)
    if full:
        for o in operands:
            for pad, off in ONE_AT_A_TIME + ([(5, 2)] if o == 'out' else []):
                if o == 'vec' and off == 0:
                    continue
                lay = {x: (0, 0) for x in operands}
                lay[o] = (pad, off)
                out.append(lay)
    return out


def lay_id(lay):
    vals = set(lay.values())
    if len(vals) == 1:
        return 'all%d.%d' % next(iter(vals))
    return ','.join('%s%d.%d' % (k, v[0], v[1]) for k, v in sorted(lay.items()) if v != (0, 0)) or 'packed'


def rnd(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------
# B. all-candidates scoring
# ---------------------------------------------------------------------------
MODES = ['dot', 'dot2', 'l2x', 'l1d', 'l2d', 'l1d_ax', 'l2d_ax', 'projh', 'projd', 'tl1', 'tl2', 'tel2']
N_REL = 5
C_BASE = 5      # global id of local candidate 0 (pair / filter kernels take GLOBAL ids)


def mode_code(hip, mode):
    return {'dot': hip.LP_DOT, 'dot2': hip.LP_DOT, 'l2x': hip.LP_L2_EXPAND, 'l1d': hip.LP_L1_DIRECT, 'l2d': hip.LP_L2_DIRECT,
            'l1d_ax': hip.LP_L1_DIRECT, 'l2d_ax': hip.LP_L2_DIRECT, 'projh': hip.LP_L2_PROJH, 'projd': hip.LP_L2_PROJD,
            'tl1': hip.LP_TORUS_L1, 'tl2': hip.LP_TORUS_L2, 'tel2': hip.LP_TORUS_EL2}[mode]


def make_ops(mode, B, N, K, seed=0):
    """Packed CPU operands of one kge_lp_desc (name -> tensor), qn / en by the oracle's chain where a mode reads them."""
    g = torch.Generator().manual_seed(1000003 * B + 1009 * N + K + seed)
    ops = {'A0': rnd(g, B, K), 'T0': rnd(g, N, K)}
    if mode in ('tl1', 'tl2', 'tel2'):
        # x = A0 - T0 in (-1, 1): every torus term is then >= 0, the sum has no cancellation, and the fp32 sum of K / 4
        # groups is within (K / 4 + 3) * 2^-24 < 1e-5 of the float64 restatement, relatively, for every K <= 512 -- the
        # TorusE tests' tolerance holds at every inner dimension of the matrix, not only at their d = 32
        ops = {'A0': ops['A0'] * 0.5, 'T0': ops['T0'] * 0.5}
    if mode == 'dot2':
        ops['A1'], ops['T1'] = rnd(g, B, K), rnd(g, N, K)
    if mode in ('l2x', 'projh', 'projd'):
        lib = oracle_clib()
        qn, en = np.empty(B, np.float32), np.empty(N, np.float32)
        lib.orc_row_sqnorm_chain(fptr(ops['A0'].numpy()), i64(K), i64(B), i64(K), fptr(qn))
        lib.orc_row_sqnorm_chain(fptr(ops['T0'].numpy()), i64(K), i64(N), i64(K), fptr(en))
        ops['qn'], ops['en'] = torch.from_numpy(qn), torch.from_numpy(en)
    if mode in ('l1d_ax', 'l2d_ax'):
        ops['Wq'], ops['scal'] = rnd(g, B, K) * 0.5, rnd(g, N, N_REL) * 0.5
        ops['r_idx'] = torch.randint(0, N_REL, (B,), generator=g)
    if mode in ('projh', 'projd'):
        ops['Wq'], ops['scal'] = rnd(g, B, 2) * 0.5, rnd(g, N_REL, N) * 0.2      # (p_i, z_i) and X (n_rel, N)
        ops['r_idx'] = torch.randint(0, N_REL, (B,), generator=g)
        if mode == 'projd':
            ops['yc'] = rnd(g, N) * 0.2
    return ops


def operand_names(mode):
    return [k for k in ('A0', 'T0', 'A1', 'T1', 'Wq', 'scal') if k in make_ops(mode, 1, 1, 1)] + ['vec', 'out']


def reference(mode, ops):
    """(scores (B, N) float32 or float64, exact): the oracle's chains on the packed arrays (bit contract), or -- the torus
    modes, for which the oracle has no chain -- the float64 restatement the TorusE tests use."""
    lib = oracle_clib()
    A0, T0 = ops['A0'].numpy(), ops['T0'].numpy()
    (B, K), N = A0.shape, T0.shape[0]
    ref = np.empty((B, N), dtype=np.float32)
    nul = None
    if mode in ('dot', 'dot2', 'l2x'):
        two = mode == 'dot2'
        lib.orc_lp_gemm_chain(fptr(A0), i64(K), fptr(T0), i64(K), i64(K), fptr(ops['A1'].numpy()) if two else nul, i64(K),
                              fptr(ops['T1'].numpy()) if two else nul, i64(K), i64(K if two else 0), i64(B), i64(N),
                              1 if mode == 'l2x' else 0, fptr(ops['qn'].numpy()) if mode == 'l2x' else nul,
                              fptr(ops['en'].numpy()) if mode == 'l2x' else nul, fptr(ref))
        return ref, True
    if mode in ('projh', 'projd'):
        yc = ops['yc'].numpy() if mode == 'projd' else np.zeros(N, np.float32)
        lib.orc_lp_proj_chain(ctypes.c_int(4 if mode == 'projh' else 5), fptr(A0), i64(K), fptr(T0), i64(K), i64(K), i64(B),
                              i64(N), fptr(ops['qn'].numpy()), fptr(ops['en'].numpy()), fptr(ops['scal'].numpy()), i64(N),
                              fptr(ops['r_idx'].numpy()), fptr(yc), fptr(ops['Wq'].numpy()), fptr(ref))
        return ref, True
    if mode in ('l1d', 'l2d', 'l1d_ax', 'l2d_ax'):
        ax = mode.endswith('_ax')
        lib.orc_lp_direct_chain(fptr(A0), i64(K), fptr(T0), i64(K), i64(K), fptr(ops['Wq'].numpy()) if ax else nul, i64(K),
                                fptr(ops['scal'].numpy()) if ax else nul, i64(N_REL),
                                fptr(ops['r_idx'].numpy()) if ax else nul, i64(B), i64(N), 1 if mode.startswith('l1') else 2,
                                fptr(ref))
        return ref, True
    x = (ops['A0'].unsqueeze(1) - ops['T0'].unsqueeze(0)).double()       # x rounded to fp32 as the engine forms it
    if mode == 'tl1':
        s = 2 * torch.minimum(x.abs(), 1 - x.abs()).sum(-1)
    elif mode == 'tl2':
        s = 4 * torch.minimum(x ** 2, 1 - x ** 2).sum(-1)
    else:
        s = (2 * (1 - torch.cos(2 * math.pi * torch.minimum(x, 1 - x)))).sum(-1) / 4
    return (-s).numpy(), False


def close(a, ref, tol=TOL):
    """|a - ref| <= tol * max(1, |ref|) (tests/test_gpu_toruse.py)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return a.size == 0 or (np.abs(a - ref) / np.maximum(1.0, np.abs(ref))).max() < tol


def problem(hip, mode, ops, lay, poison=NAN, c_base=0):
    """hip.LpProblem on carved device operands: matrices by lay[name] = (pad, off), 1-D float vectors at lay['vec'][1]
    floats, int64 vectors at one element (8 bytes) when that offset is odd.  r_idx is poisoned with a relation id one
    past the last: a kernel that read it would fetch the NaN slack row / column of `scal`."""
    dv = {}
    voff = lay.get('vec', (0, 0))[1]
    for name, t in ops.items():
        if t.dtype == torch.int64:
            dv[name] = carve(t, off=voff % 2, poison=N_REL, device='cuda')
        elif t.dim() == 1:
            dv[name] = carve(t, off=voff, poison=poison, device='cuda')
        else:
            pad, off = lay.get(name, (0, 0))
            dv[name] = carve(t, pad, off, poison, device='cuda')
    prob = hip.LpProblem(mode_code(hip, mode), dv['A0'], dv['T0'], A1=dv.get('A1'), T1=dv.get('T1'), qn=dv.get('qn'),
                         en=dv.get('en'), Wq=dv.get('Wq'), scal=dv.get('scal'), r_idx=dv.get('r_idx'), c_base=c_base,
                         yc=dv.get('yc'))
    d, K = prob.desc, ops['A0'].shape[1]
    assert (d.lda0, d.ldt0) == (K + lay.get('A0', (0, 0))[0], K + lay.get('T0', (0, 0))[0])
    assert d.A0 % 16 == 4 * lay.get('A0', (0, 0))[1] and d.T0 % 16 == 4 * lay.get('T0', (0, 0))[1]
    return prob, dv


def scores_into_guard(hip, prob, lay):
    B, N = prob.B, prob.N
    pad, off = lay.get('out', (0, 0))
    out = guarded_out(B, N, pad, off)
    rc = raw(hip.load_library(), 'kge_lp_scores', prob.desc, out, out.stride(0))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guard_intact(out)
    return out


def packed_scores(hip, mode, ops):
    """The base call: packed, aligned operands (still carved: poison around them), checked against the reference."""
    prob, dv = problem(hip, mode, ops, {})
    S = scores_into_guard(hip, prob, {}).clone()
    ref, exact = reference(mode, ops)
    got = S.cpu().numpy()
    assert np.isfinite(got).all()
    if exact:
        assert np.array_equal(got, ref)
    else:
        assert close(got, ref)
    return S


def check_scores(hip, mode, ops, lay, S):
    prob, dv = problem(hip, mode, ops, lay)
    out = scores_into_guard(hip, prob, lay)
    assert bool(torch.isfinite(out).all()), 'poison reached the scores'
    assert same_bits(out, S)
    for v in dv.values():
        assert_guard_intact(v)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B,N,K', SMALL)
def test_lp_scores_every_layout_at_the_small_shapes(hip, mode, B, N, K):
    """kge_lp_scores, every mode of kge_lp_desc, every layout of the matrix (one operand at a time and all at once), into
    a guarded output with ldo in {N, N + 1, N + 4, N + 5} at offsets 0..3."""
    ops = make_ops(mode, B, N, K)
    S = packed_scores(hip, mode, ops)
    for lay in layouts(operand_names(mode)):
        try:
            check_scores(hip, mode, ops, lay, S)
        except AssertionError as e:
            raise AssertionError('%s layout %s: %s' % (mode, lay_id(lay), e))


@pytest.mark.parametrize('mode', MODES)
def test_lp_scores_few_layouts_at_every_shape(hip, mode):
    """The same at every inner dimension and on both sides of the kernels' row / candidate tiles, plus the TransD form
    (K0 = 48 inside ldt0 = 72)."""
    for B, N, K in SHAPES:
        ops = make_ops(mode, B, N, K)
        S = packed_scores(hip, mode, ops)
        lays = layouts(operand_names(mode), full=False)
        if K == 48:
            lays.append({'T0': (24, 0)})
            lays.append({'T0': (24, 0), 'A0': (0, 1)})
        for lay in lays:
            try:
                check_scores(hip, mode, ops, lay, S)
            except AssertionError as e:
                raise AssertionError('%s (%d, %d, %d) layout %s: %s' % (mode, B, N, K, lay_id(lay), e))


def filter_fixture(g, B, N, true_loc):
    """Filter segments over GLOBAL ids (some outside the shard [C_BASE, C_BASE + N)), one distinct non-empty segment per
    query (so the precondition of the grouped / planned forms holds), about half of them holding the true entity."""
    lo, hi, tg = [], [], []
    for i in range(B):
        n = int(torch.randint(1, 7, (1,), generator=g))
        ids = torch.randint(0, N + 2 * C_BASE, (n,), generator=g).tolist()
        if i % 2 == 0:
            ids[int(torch.randint(0, n, (1,), generator=g))] = int(true_loc[i]) + C_BASE
        ids = sorted(set(ids))
        lo.append(len(tg))
        tg.extend(ids)
        hi.append(len(tg))
    return (torch.tensor(lo, dtype=torch.int64), torch.tensor(hi, dtype=torch.int64), torch.tensor(tg, dtype=torch.int32))


def filter_expect(S, st, true_glob, lo, hi, tg, N):
    """sub / found of kge_lp_filter_sub from the (B, N) score matrix (include/kge_hip.h)."""
    B = S.shape[0]
    sub, found = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for i in range(B):
        neg = 1 if -INF >= st[i] else 0
        for gid in tg[int(lo[i]):int(hi[i])].tolist():
            c = gid - C_BASE
            if c < 0 or c >= N:
                continue
            if gid == int(true_glob[i]):
                found[i] = 1
                continue
            sub[i] += int(S[i, c] >= st[i]) - neg
    return sub, found


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B,N,K', [(33, 193, 17), (65, 257, 64), (129, 192, 8)])
def test_pair_count_and_filter_kernels_on_carved_descriptors(hip, mode, B, N, K):
    """kge_lp_pair_scores, kge_lp_count_ge, kge_lp_filter_sub and its grouped / planned forms on carved descriptors: the
    pair scores are the bits of the score matrix, counts and filter corrections the integers that matrix gives."""
    lib = hip.load_library()
    ops = make_ops(mode, B, N, K)
    S = packed_scores(hip, mode, ops).cpu().numpy()
    g = torch.Generator().manual_seed(B + N + K)
    true_loc = torch.randint(0, N, (B,), generator=g)
    st = S[np.arange(B), true_loc.numpy()]
    # pairs: every query's true entity, then explicit (query, candidate) pairs, a few ids outside the shard (-> 0)
    P = B + 40
    qi = torch.cat([torch.arange(B), torch.randint(0, B, (40,), generator=g)])
    ci = torch.cat([true_loc + C_BASE, torch.randint(0, N + 2 * C_BASE, (40,), generator=g)])
    loc = ci - C_BASE
    inside = (loc >= 0) & (loc < N)
    pair_ref = np.where(inside.numpy(), S[qi.numpy(), loc.clamp(0, N - 1).numpy()], np.float32(0))
    lo, hi, tg = filter_fixture(g, B, N, true_loc)
    sub_ref, found_ref = filter_expect(S, st, true_loc + C_BASE, lo, hi, tg, N)
    cnt_ref = (S >= st[:, None]).sum(1).astype(np.int32)
    names = [n for n in operand_names(mode) if n != 'out']
    for lay in layouts(names, full=(B == 33)):
        prob, dv = problem(hip, mode, ops, lay, c_base=C_BASE)
        voff = lay['vec'][1]
        tag = '%s layout %s' % (mode, lay_id(lay))
        # ids one past the shard as poison: a kernel that read them would score the NaN slack rows
        d_ci = carve(ci, off=voff % 2, poison=N + C_BASE, device='cuda')
        d_qi = carve(qi, off=(voff + 1) % 2, poison=0, device='cuda')
        po = guarded_out(P, off=voff)
        assert raw(lib, 'kge_lp_pair_scores', prob.desc, d_qi, d_ci, P, po) == 0, tag
        p1 = guarded_out(B, off=(voff + 1) % 4)
        assert raw(lib, 'kge_lp_pair_scores', prob.desc, None, d_ci, B, p1) == 0, tag      # qi == NULL: qi[p] = p
        d_st = carve(torch.from_numpy(st.copy()), off=voff, poison=NAN, device='cuda')
        cnt = guarded_out(B, off=(voff + 2) % 4, dtype=torch.int32)
        cnt.zero_()
        assert raw(lib, 'kge_lp_count_ge', prob.desc, d_st, cnt) == 0, tag
        d_true = carve(true_loc + C_BASE, off=voff % 2, poison=N + C_BASE, device='cuda')
        d_lo, d_hi = carve(lo, off=(voff + 1) % 2, poison=0, device='cuda'), carve(hi, off=voff % 2, poison=0, device='cuda')
        d_tg = carve(tg, off=voff, poison=N + C_BASE, device='cuda')
        res = []
        for form in ('plain', 'grouped', 'planned'):
            sub, found = guarded_out(B, off=voff, dtype=torch.int32), guarded_out(B, off=(voff + 3) % 4, dtype=torch.int32)
            n_t = int(tg.shape[0])
            if form == 'plain':
                rc = raw(lib, 'kge_lp_filter_sub', prob.desc, d_st, d_true, d_lo, d_hi, d_tg, sub, found)
            elif form == 'grouped':
                nb = int(lib.kge_lp_filter_sub_ws_bytes(B, n_t))
                ws = torch.empty(max(nb, 8), dtype=torch.uint8, device='cuda')
                rc = raw(lib, 'kge_lp_filter_sub_grouped', prob.desc, d_st, d_true, d_lo, d_hi, d_tg, n_t, sub, found, ws, nb)
            else:
                woff, long_q, n_pairs = hip.filter_plan_build(d_lo, d_hi, n_t, 512)
                fs = guarded_out(n_t, off=voff)
                rc = raw(lib, 'kge_lp_filter_sub_planned', prob.desc, d_st, d_true, d_lo, d_hi, d_tg, n_t, woff, n_pairs,
                         None, 0, fs, sub, found)
                assert int(long_q.shape[0]) == 0
                res.append(fs)
            assert rc == 0, (tag, form)
            res += [sub, found]
            torch.cuda.synchronize()
            assert np.array_equal(sub.cpu().numpy(), sub_ref), (tag, form)
            assert np.array_equal(found.cpu().numpy(), found_ref), (tag, form)
        torch.cuda.synchronize()
        got = po.cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got.view(np.int32), pair_ref.astype(np.float32).view(np.int32)), tag
        assert np.array_equal(p1.cpu().numpy().view(np.int32), st.view(np.int32)), tag
        assert np.array_equal(cnt.cpu().numpy(), cnt_ref), tag
        for v in [po, p1, cnt, d_ci, d_qi, d_st, d_true, d_lo, d_hi, d_tg] + res + list(dv.values()):
            assert_guard_intact(v)


PAIR_GRID_CAP = 256 * 14        # blocks of the pair kernels (one wavefront, 64 pairs per round): past it a block loops


@pytest.mark.parametrize('mode', ['dot', 'l2d', 'l1d_ax', 'tel2'])
@pytest.mark.parametrize('K', [17, 64])
def test_pair_scores_past_the_grid_cap(hip, mode, K):
    """kge_lp_pair_scores with more 64-pair groups than the grid has blocks (the first blocks take a second round, the
    last group is partial): every output is the bits of the score matrix at (qi, ci), 0 outside the shard.  K = 64 runs
    the staged chains on float4 rows (dot, L2 direct, torus eL2), K = 17 the staged dot chain on unaligned rows and the
    scalar walk; l1d_ax the scalar walk with the rank-1 term."""
    lib = hip.load_library()
    B, N = 65, 193
    P = 64 * PAIR_GRID_CAP + 65
    ops = make_ops(mode, B, N, K)
    S = packed_scores(hip, mode, ops).cpu().numpy()
    g = torch.Generator().manual_seed(P + K)
    qi = torch.randint(0, B, (P,), generator=g)
    ci = torch.randint(0, N + 2 * C_BASE, (P,), generator=g)        # GLOBAL ids, a few outside [C_BASE, C_BASE + N)
    loc = ci - C_BASE
    inside = (loc >= 0) & (loc < N)
    assert 0 < int((~inside).sum()) < P // 10
    ref = np.where(inside.numpy(), S[qi.numpy(), loc.clamp(0, N - 1).numpy()], np.float32(0)).astype(np.float32)
    prob, dv = problem(hip, mode, ops, {}, c_base=C_BASE)
    d_qi, d_ci = carve(qi, poison=0, device='cuda'), carve(ci, poison=N + C_BASE, device='cuda')
    out = guarded_out(P)
    assert raw(lib, 'kge_lp_pair_scores', prob.desc, d_qi, d_ci, P, out) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int32), ref.view(np.int32))
    for v in [out, d_qi, d_ci] + list(dv.values()):
        assert_guard_intact(v)


def filter_expect_dense(S, st, true_glob, tg2d, N):
    """filter_expect for segments of one length, vectorised: tg2d (B, L) holds query i's segment."""
    c = tg2d - C_BASE
    inside = (c >= 0) & (c < N)
    is_true = tg2d == true_glob[:, None]
    ge = np.take_along_axis(S, np.clip(c, 0, N - 1), 1) >= st[:, None]
    neg = (-INF >= st).astype(np.int32)
    sub = ((ge.astype(np.int32) - neg[:, None]) * (inside & ~is_true)).sum(1).astype(np.int32)
    return sub, (inside & is_true).any(1).astype(np.int32)


@pytest.mark.parametrize('mode', ['dot', 'l1d'])
def test_planned_filter_correction_past_the_grid_cap(hip, mode):
    """kge_lp_filter_sub_planned with more flattened (key, target) pairs than 64 per block of the scoring grid: 600
    queries with distinct segments of 400 targets (below the hub-list length, so the short compare runs), sub / found
    the integers the score matrix gives."""
    lib = hip.load_library()
    B, N, K, L = 600, 512, 64, 400
    assert B * L > 64 * PAIR_GRID_CAP
    ops = make_ops(mode, B, N, K)
    S = packed_scores(hip, mode, ops).cpu().numpy()
    g = torch.Generator().manual_seed(B + N + L)
    true_loc = torch.randint(0, N, (B,), generator=g)
    st = S[np.arange(B), true_loc.numpy()]
    tg2d = torch.stack([torch.randperm(N + 2 * C_BASE, generator=g)[:L] for _ in range(B)])     # distinct GLOBAL ids
    for i in range(0, B, 2):            # every other segment holds its query's true entity
        if not bool((tg2d[i] == true_loc[i] + C_BASE).any()):
            tg2d[i, 0] = true_loc[i] + C_BASE
    tg2d = tg2d.sort(1).values
    lo = torch.arange(B, dtype=torch.int64) * L
    hi, tg = lo + L, tg2d.reshape(-1).to(torch.int32)
    true_glob = (true_loc + C_BASE).numpy()
    sub_ref, found_ref = filter_expect_dense(S, st, true_glob, tg2d.numpy(), N)
    few = filter_expect(S[:8], st[:8], true_loc[:8] + C_BASE, lo[:8], hi[:8], tg, N)        # the vectorised form is the loop's
    assert np.array_equal(few[0], sub_ref[:8]) and np.array_equal(few[1], found_ref[:8])
    assert 0 < int(found_ref.sum()) < B and int(np.abs(sub_ref).sum()) > 0
    prob, dv = problem(hip, mode, ops, {}, c_base=C_BASE)
    d_st = carve(torch.from_numpy(st.copy()), poison=NAN, device='cuda')
    d_true = carve(true_loc + C_BASE, poison=N + C_BASE, device='cuda')
    d_lo, d_hi = carve(lo, poison=0, device='cuda'), carve(hi, poison=0, device='cuda')
    d_tg = carve(tg, poison=N + C_BASE, device='cuda')
    n_t = B * L
    woff, long_q, n_pairs = hip.filter_plan_build(d_lo, d_hi, n_t, 512)
    assert n_pairs == n_t and int(long_q.shape[0]) == 0
    fs = guarded_out(n_t)
    sub, found = guarded_out(B, dtype=torch.int32), guarded_out(B, dtype=torch.int32)
    rc = raw(lib, 'kge_lp_filter_sub_planned', prob.desc, d_st, d_true, d_lo, d_hi, d_tg, n_t, woff, n_pairs, None, 0, fs, sub,
             found)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(sub.cpu().numpy(), sub_ref)
    assert np.array_equal(found.cpu().numpy(), found_ref)
    for v in [fs, sub, found, d_st, d_true, d_lo, d_hi, d_tg] + list(dv.values()):
        assert_guard_intact(v)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('K', [8, 17])
def test_pointer_advancing_chunks_and_row_blocks_equal_the_slices(hip, mode, K):
    """LpProblem.scores_chunk(c0, c1) / scores_rows(q0, q1) -- the descriptor with its candidate-side / query-side
    pointers advanced by an arbitrary number of elements (en, yc and, in the projection modes, the COLUMNS of scal land
    off a 16-byte boundary) -- equal the slices of the full matrix bit for bit."""
    B, N = 37, 300
    ops = make_ops(mode, B, N, K)
    S = packed_scores(hip, mode, ops)
    for lay in layouts([n for n in operand_names(mode)], full=False):
        prob, dv = problem(hip, mode, ops, lay)
        pad, off = lay['out']
        for c0 in (1, 7, 255, 257):
            for c1 in (N, min(N, c0 + 31)):
                out = guarded_out(B, c1 - c0, pad + 3, off)        # (as the tiled top-k calls it: ldo > c1 - c0)
                prob.scores_chunk(c0, c1, out)
                torch.cuda.synchronize()
                assert same_bits(out, S[:, c0:c1]), (mode, lay_id(lay), c0, c1)
                assert_guard_intact(out)
        for q0, q1 in ((1, B), (33, B), (3, 4), (0, 17)):
            out = guarded_out(q1 - q0, N, pad, off)
            prob.scores_rows(q0, q1, out)
            torch.cuda.synchronize()
            assert same_bits(out, S[q0:q1]), (mode, lay_id(lay), q0, q1)
            assert_guard_intact(out)
        for v in dv.values():
            assert_guard_intact(v)


# ---------------------------------------------------------------------------
# G. rank / filter / top-k on a materialised score matrix
# ---------------------------------------------------------------------------
RANK_SHAPES = [(1, 1), (5, 3), (33, 193), (7, 255), (6, 256), (9, 257), (4, 1023), (3, 1025), (64, 129)]
RANK_LAYOUTS = [(0, 0), (1, 0), (3, 0), (4, 0), (8, 0), (0, 1), (0, 2), (0, 3), (1, 1), (3, 2), (4, 3), (1, 3), (5, 2)]


def score_matrix(g, B, N):
    """Scores with many exact ties (the rank compares are >= / <=) and a few -inf entries."""
    S = torch.randint(-40, 40, (B, N), generator=g).float() / 8
    S[torch.rand(B, N, generator=g) < 0.02] = -INF
    return S


def csr_fixture(g, B, N):
    """Per-query filter segments (LOCAL ids): empty ones, ones without the true entity, ones with it."""
    true = torch.randint(0, N, (B,), generator=g)
    has, off, tgt = [], [0], []
    for i in range(B):
        kind = i % 4
        ids = set(torch.randint(0, N, (int(torch.randint(1, 9, (1,), generator=g)),), generator=g).tolist())
        if kind == 0:
            ids = set()
        elif kind == 1:
            ids.discard(int(true[i]))
        else:
            ids.add(int(true[i]))
        has.append(1 if ids else 0)
        tgt.extend(sorted(ids))
        off.append(len(tgt))
    return true, np.array(has, np.uint8), np.array(off, np.int64), np.array(tgt, np.int64)


@pytest.mark.parametrize('B,N', RANK_SHAPES)
def test_rank_and_filter_kernels_on_carved_score_matrices(hip, B, N):
    """kge_get_rank (whose 16-byte head peel meets another remainder on every row when ld is odd), kge_filter_scores (in
    place: pad intact), kge_filtered_rank_from_scores: integers equal to the oracle's on the packed matrix, with NaN,
    +inf and -inf in the pads (a pad read would change a count)."""
    lib, orc = hip.load_library(), oracle_clib()
    g = torch.Generator().manual_seed(B * 7 + N)
    S = score_matrix(g, B, N)
    true, has, off, tgt = csr_fixture(g, B, N)
    Sn, tn = S.numpy(), true.numpy()
    rk_ref = {}
    for low in (0, 1):
        rk_ref[low] = np.empty(B, np.int64)
        orc.orc_get_rank(fptr(Sn), fptr(tn), i64(B), i64(N), low, fptr(rk_ref[low]))
    filt_ref = Sn.copy()
    orc.orc_filter_scores(fptr(filt_ref), i64(B), i64(N), fptr(tn), fptr(has), fptr(off), fptr(tgt))
    all_ref = Sn.copy()         # true_idx == NULL: every listed target is masked
    for i in range(B):
        all_ref[i, tgt[off[i]:off[i + 1]]] = -INF
    r_ref, f_ref = np.empty(B, np.int64), np.empty(B, np.int64)
    orc.orc_filtered_rank(fptr(Sn), i64(B), i64(N), fptr(tn), fptr(has), fptr(off), fptr(tgt), fptr(r_ref), fptr(f_ref))
    lo, hi = torch.from_numpy(off[:-1].copy()), torch.from_numpy(off[1:].copy())
    tg32 = torch.from_numpy(tgt.astype(np.int32))
    for pad, o in RANK_LAYOUTS:
        for poison in (NAN, INF, -INF):
            tag = 'pad %d off %d poison %r' % (pad, o, poison)
            d_S = carve(S, pad, o, poison, device='cuda')
            d_true = carve(true, off=o % 2, poison=N, device='cuda')       # (column N: the first pad / slack element)
            d_lo, d_hi = carve(lo, off=(o + 1) % 2, poison=0, device='cuda'), carve(hi, off=o % 2, poison=0, device='cuda')
            d_tg = carve(tg32, off=o, poison=N, device='cuda')
            outs = []
            for low in (0, 1):
                rk = guarded_out(B, off=(o + low) % 2, dtype=torch.int64)
                assert raw(lib, 'kge_get_rank', d_S, d_S.stride(0), d_true, B, N, low, rk) == 0, tag
                torch.cuda.synchronize()
                assert np.array_equal(rk.cpu().numpy(), rk_ref[low]), (tag, low)
                outs.append(rk)
            rk, fk = guarded_out(B, off=o % 2, dtype=torch.int64), guarded_out(B, off=(o + 1) % 2, dtype=torch.int64)
            assert raw(lib, 'kge_filtered_rank_from_scores', d_S, d_S.stride(0), d_true, d_lo, d_hi, d_tg, B, N, rk, fk) == 0, tag
            torch.cuda.synchronize()
            assert np.array_equal(rk.cpu().numpy(), r_ref) and np.array_equal(fk.cpu().numpy(), f_ref), tag
            assert_guard_intact(d_S)        # read-only so far
            assert raw(lib, 'kge_filter_scores', d_S, d_S.stride(0), d_true, d_lo, d_hi, d_tg, B, N) == 0, tag
            torch.cuda.synchronize()
            assert np.array_equal(d_S.cpu().numpy(), filt_ref), tag
            d_S2 = carve(S, pad, o, poison, device='cuda')
            assert raw(lib, 'kge_filter_scores', d_S2, d_S2.stride(0), None, d_lo, d_hi, d_tg, B, N) == 0, tag
            torch.cuda.synchronize()
            assert np.array_equal(d_S2.cpu().numpy(), all_ref), tag
            for v in outs + [rk, fk, d_S, d_S2, d_true, d_lo, d_hi, d_tg]:
                assert_guard_intact(v)


def topk_ref(S, k):
    """(values, column indices) of the k best per row in the order (score descending, index ascending)."""
    B, N = S.shape
    idx = np.empty((B, k), np.int64)
    for i in range(B):
        idx[i] = np.lexsort((np.arange(N), -S[i].astype(np.float64)))[:k]
    return np.take_along_axis(S, idx, 1), idx


@pytest.mark.parametrize('B,N,k', [(5, 3, 3), (7, 300, 5), (4, 1000, 1), (3, 1025, 10), (9, 257, 32), (2, 4097, 40), (6, 64, 8)])
def test_topk_kernels_on_carved_score_matrices(hip, B, N, k):
    """kge_topk on a strided matrix, and kge_topk_chunk as the tiled inference calls it: the live tile is the first C
    columns of a wider scratch matrix (ld > C), the k best land in columns [col_off, col_off + k) of (B, ldo) outputs.
    +inf in a pad would be selected first, NaN never: both poisons, values and ids exact."""
    lib = hip.load_library()
    g = torch.Generator().manual_seed(B + N + k)
    S = score_matrix(g, B, N)
    v_ref, i_ref = topk_ref(S.numpy(), k)
    true, has, off, tgt = csr_fixture(g, B, N)
    masked = S.numpy().copy()
    for i in range(B):
        masked[i, tgt[off[i]:off[i + 1]]] = -INF
    vm_ref, im_ref = topk_ref(masked, k)
    lo, hi = torch.from_numpy(off[:-1].copy()), torch.from_numpy(off[1:].copy())
    ids = torch.arange(N).view(1, N).repeat(B, 1) * 3 + 7            # merge mode: ascending candidate ids, some padding
    if N >= 4 * k:
        ids[torch.rand(B, N, generator=g) < 0.2] = -1
    mi_ref, mv_ref = np.empty((B, k), np.int64), np.empty((B, k), np.float32)
    for i in range(B):
        cols = np.nonzero(ids[i].numpy() >= 0)[0]
        best = cols[np.lexsort((cols, -S[i].numpy()[cols].astype(np.float64)))[:k]]
        mi_ref[i], mv_ref[i] = ids[i].numpy()[best], S[i].numpy()[best]
    c_base, col_off = 1000, 3
    tg32 = torch.from_numpy((tgt + c_base).astype(np.int32))
    for pad, o in RANK_LAYOUTS:
        for poison in (NAN, INF):
            tag = 'pad %d off %d poison %r' % (pad, o, poison)
            d_S = carve(S, pad, o, poison, device='cuda')
            idx, val = guarded_out(B, k, 0, o % 2, dtype=torch.int64), guarded_out(B, k, 0, (o + 1) % 4)
            assert raw(lib, 'kge_topk', d_S, d_S.stride(0), B, N, k, idx, val) == 0, tag
            torch.cuda.synchronize()
            assert np.array_equal(idx.cpu().numpy(), i_ref), tag
            assert np.array_equal(val.cpu().numpy().view(np.int32), v_ref.view(np.int32)), tag
            # the chunk form: unfiltered, then with the rows' filter segments masked in place (GLOBAL ids)
            for filt in (False, True):
                d_T = carve(S, pad + 2, o, poison, device='cuda')
                d_lo, d_hi = carve(lo, off=o % 2, poison=0, device='cuda'), carve(hi, off=(o + 1) % 2, poison=0, device='cuda')
                d_tg = carve(tg32, off=o, poison=c_base + N, device='cuda')
                ldo_pad = pad + 1
                cidx = guarded_out(B, col_off + k, ldo_pad, o % 2, dtype=torch.int64)
                cval = guarded_out(B, col_off + k, ldo_pad, (o + 2) % 4)
                ldv = cval.stride(0)
                # (idx and val share ldo: the int64 matrix is laid out with the same number of ELEMENTS per row)
                assert cidx.stride(0) == ldv
                rc = raw(lib, 'kge_topk_chunk', d_T, d_T.stride(0), B, N, c_base, k, d_lo if filt else None,
                         d_hi if filt else None, d_tg if filt else None, None, 0, cidx, cval, ldv, col_off)
                assert rc == 0, tag
                torch.cuda.synchronize()
                ir, vr = (im_ref, vm_ref) if filt else (i_ref, v_ref)
                assert np.array_equal(cidx[:, col_off:].cpu().numpy(), ir + c_base), (tag, filt)
                assert np.array_equal(cval[:, col_off:].cpu().numpy().view(np.int32), vr.view(np.int32)), (tag, filt)
                assert np.array_equal(d_T.cpu().numpy(), masked if filt else S.numpy()), (tag, filt)
                assert_guard_intact(cidx, col0=col_off)
                assert_guard_intact(cval, col0=col_off)
                for v in (d_T, d_lo, d_hi, d_tg):
                    assert_guard_intact(v)
            # merge mode: column c stands for candidate ids_in[i * ld_ids + c] (ld_ids > C), ids < 0 are padding
            d_M = carve(S, pad + 1, o, poison, device='cuda')
            d_ids = carve(ids, pad + 3, o % 2, poison=10 ** 9, device='cuda')
            midx, mval = guarded_out(B, k, 2, (o + 1) % 2, dtype=torch.int64), guarded_out(B, k, 2, (o + 3) % 4)
            assert raw(lib, 'kge_topk_chunk', d_M, d_M.stride(0), B, N, 0, k, None, None, None, d_ids, d_ids.stride(0), midx, mval,
                       mval.stride(0), 0) == 0, tag
            torch.cuda.synchronize()
            assert np.array_equal(midx.cpu().numpy(), mi_ref), tag
            assert np.array_equal(mval.cpu().numpy().view(np.int32), mv_ref.view(np.int32)), tag
            for v in (d_S, idx, val, d_M, d_ids, midx, mval):
                assert_guard_intact(v)


@pytest.mark.parametrize('Bf,N,world', [(5, 17, 1), (33, 193, 3), (64, 257, 2), (9, 1000, 4)])
def test_rank_from_tiles_and_finalize_into_a_guarded_result_matrix(hip, Bf, N, world):
    """kge_filtered_rank_from_tiles (rank-major tiles, packed by contract: the layout axis is the base offset) and
    kge_rank_finalize_both, both into a (4, ld) result matrix with ld > off + B, off > 0 and a `pos` scatter: only the
    addressed elements change, and they hold the oracle's ranks."""
    lib, orc = hip.load_library(), oracle_clib()
    g = torch.Generator().manual_seed(Bf + N + world)
    B2 = 2 * Bf                                 # a both-sides batch: tail-side queries first
    S = score_matrix(g, B2, N)
    true, has, off, tgt = csr_fixture(g, B2, N)
    r_ref, f_ref = np.empty(B2, np.int64), np.empty(B2, np.int64)
    orc.orc_filtered_rank(fptr(S.numpy()), i64(B2), i64(N), fptr(true.numpy()), fptr(has), fptr(off), fptr(tgt), fptr(r_ref),
                          fptr(f_ref))
    per = (N + world - 1) // world
    m = B2 + 3
    tiles = torch.full((world, m, per), 1e30)       # rows >= B2 and columns >= N of the last tile are never read
    for p in range(world):
        w = min(per, N - p * per)
        tiles[p, :B2, :w] = S[:, p * per:p * per + w]
    lo, hi = torch.from_numpy(off[:-1].copy()), torch.from_numpy(off[1:].copy())
    tg32 = torch.from_numpy(tgt.astype(np.int32))
    sentinel = int(guarded_out(1, dtype=torch.int64, device='cpu')[0])
    col0 = 2
    perm = torch.randperm(col0 + Bf, generator=g)
    for o in range(4):
        for use_pos in (False, True):
            for poison in (NAN, INF):
                tag = 'off %d pos %s poison %r' % (o, use_pos, poison)
                d_tiles = carve(tiles.view(-1), off=o, poison=poison, device='cuda')
                d_true = carve(true, off=o % 2, poison=N, device='cuda')
                d_lo, d_hi = carve(lo, off=(o + 1) % 2, poison=0, device='cuda'), carve(hi, off=o % 2, poison=0, device='cuda')
                d_tg = carve(tg32, off=o, poison=N, device='cuda')
                d_pos = carve(perm, off=o % 2, poison=0, device='cuda') if use_pos else None
                ncol = col0 + Bf
                expect = np.full((4, ncol), sentinel, np.int64)
                for q in range(B2):
                    tail = q < Bf
                    j = col0 + (q if tail else q - Bf)
                    f = int(perm[j]) if use_pos else j
                    expect[1 if tail else 0, f], expect[3 if tail else 2, f] = r_ref[q], f_ref[q]
                out = guarded_out(4, ncol, 3, o % 2, dtype=torch.int64)
                rows0 = 7               # two calls: a row block, then the rest (q_first > 0).  Row i of every tile belongs
                # to query q_first + i, so the second call gets the tiles ADVANCED by q_first rows (same m: the tile
                # stride), which also moves their base by an odd number of floats
                for q_first, rows in ((0, rows0), (rows0, B2 - rows0)):
                    rc = raw(lib, 'kge_filtered_rank_from_tiles', d_tiles[q_first * per:], m, per, world, N,
                             d_true[q_first:], d_lo[q_first:], d_hi[q_first:], d_tg, rows, q_first, Bf, out, out.stride(0),
                             col0, d_pos, None, 0)
                    assert rc == 0, tag
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), expect), tag
                assert_guard_intact(out)
                # `own`: tile own_rank is read from a buffer of its own (m, per), carved at another offset; that tile of
                # `tiles` holds poison to show it is never read
                own_rank = world - 1
                d_own = carve(tiles[own_rank].reshape(-1), off=(o + 1) % 4, poison=poison, device='cuda')
                t2 = tiles.clone()
                t2[own_rank] = poison
                d_t2 = carve(t2.view(-1), off=(o + 2) % 4, poison=poison, device='cuda')
                out3 = guarded_out(4, ncol, 1, (o + 1) % 2, dtype=torch.int64)
                for q_first, rows in ((0, rows0), (rows0, B2 - rows0)):
                    rc = raw(lib, 'kge_filtered_rank_from_tiles', d_t2[q_first * per:], m, per, world, N, d_true[q_first:],
                             d_lo[q_first:], d_hi[q_first:], d_tg, rows, q_first, Bf, out3, out3.stride(0), col0, d_pos,
                             d_own[q_first * per:], own_rank)
                    assert rc == 0, tag
                torch.cuda.synchronize()
                assert np.array_equal(out3.cpu().numpy(), expect), tag
                for v in (out3, d_own, d_t2):
                    assert_guard_intact(v)
                # kge_rank_finalize_both: raw / sub / found of the 2B queries -> the same matrix layout
                raw_c = torch.from_numpy(r_ref.astype(np.int32))
                found = torch.from_numpy((r_ref != f_ref).astype(np.int32))
                sub = torch.from_numpy((r_ref - f_ref).astype(np.int32))
                d_raw, d_sub = carve(raw_c, off=o, poison=-7, device='cuda'), carve(sub, off=(o + 1) % 4, poison=-7, device='cuda')
                d_found = carve(found, off=(o + 2) % 4, poison=-7, device='cuda')
                out2 = guarded_out(4, ncol, 5, (o + 1) % 2, dtype=torch.int64)
                rc = raw(lib, 'kge_rank_finalize_both', d_raw, d_sub, d_found, Bf, out2, out2.stride(0), col0, d_pos, None, None,
                         0, None)
                assert rc == 0, tag
                torch.cuda.synchronize()
                assert np.array_equal(out2.cpu().numpy(), expect), tag
                assert_guard_intact(out2)
                for v in (d_tiles, d_true, d_lo, d_hi, d_tg, d_raw, d_sub, d_found):
                    assert_guard_intact(v)


# ---------------------------------------------------------------------------
# A. row primitives
# ---------------------------------------------------------------------------
ROW_LAYOUTS = [(0, 0), (1, 0), (3, 0), (4, 0), (8, 0), (0, 1), (0, 2), (0, 3), (1, 1), (3, 2), (4, 3), (8, 1)]
ROW_COUNTS = [1, 15, 16, 17, 63, 64, 65, 257]


def _row_cases():
    for K in INNER:
        yield 33, K, ROW_LAYOUTS
    for rows in ROW_COUNTS:
        for K in (8, 17):
            yield rows, K, FEW
    yield 5, 48, [(24, 0), (24, 1)]         # the TransD form: K = 48 inside ld = 72


@pytest.mark.parametrize('rows,K,lays', list(_row_cases()), ids=lambda v: str(v) if isinstance(v, int) else 'lays')
def test_row_primitives_on_carved_matrices(hip, rows, K, lays):
    """kge_row_sqnorm (with max_io), kge_row_sqnorm_any_order, kge_row_dot, kge_gather_rows, kge_normalize_rows and
    kge_frac_rows (in place: pad intact) with explicit leading dimensions, NaN in every pad."""
    lib, orc = hip.load_library(), oracle_clib()
    g = torch.Generator().manual_seed(rows * 1000 + K)
    X, Y = rnd(g, rows, K) * 2, rnd(g, rows, K)
    n_ref, d_ref = np.empty(rows, np.float32), np.empty(rows, np.float32)
    orc.orc_row_sqnorm_chain(fptr(X.numpy()), i64(K), i64(rows), i64(K), fptr(n_ref))
    orc.orc_row_dot_chain(fptr(X.numpy()), i64(K), fptr(Y.numpy()), i64(K), i64(rows), i64(K), ctypes.c_float(-2.0), fptr(d_ref))
    n64 = (X.double() ** 2).sum(1).numpy()
    idx = torch.cat([torch.tensor([0, rows - 1, 0, rows - 1]), torch.randint(0, rows, (rows + 3,), generator=g)])
    norm64 = (X.double() / X.double().norm(dim=1, keepdim=True).clamp_min(1e-12)).numpy()
    frac_ref = (X * 3 - (X * 3).trunc()).numpy()
    base = {}
    for pad, o in [(0, 0)] + lays:
        tag = 'pad %d off %d' % (pad, o)
        ld = K + pad
        d_X = carve(X, pad, o, NAN, device='cuda')
        d_Y = carve(Y, pad, {0: 0, 1: 0, 2: 3, 3: 3}[o], NAN, device='cuda')     # X and Y share ld, not the offset
        got = {}
        mx = guarded_out(2, off=o)
        mx.zero_()
        got['sq'] = guarded_out(rows, off=o)
        assert raw(lib, 'kge_row_sqnorm', d_X, ld, rows, K, got['sq'], mx[0:1]) == 0, tag
        got['any'] = guarded_out(rows, off=(o + 1) % 4)
        assert raw(lib, 'kge_row_sqnorm_any_order', d_X, ld, rows, K, got['any'], mx[1:2]) == 0, tag
        got['dot'] = guarded_out(rows, off=(o + 2) % 4)
        assert raw(lib, 'kge_row_dot', d_X, d_Y, ld, rows, K, ctypes.c_float(-2.0), got['dot']) == 0, tag
        got['dot_yx'] = guarded_out(rows, off=(o + 3) % 4)      # operands swapped (fmaf(x, y, .) == fmaf(y, x, .)): X aligned, Y not
        assert raw(lib, 'kge_row_dot', d_Y, d_X, ld, rows, K, ctypes.c_float(-2.0), got['dot_yx']) == 0, tag
        d_idx = carve(idx, off=o % 2, poison=rows, device='cuda')       # (row `rows`: NaN slack)
        got['gather'] = guarded_out(idx.shape[0], K, 0, (o + 3) % 4)
        assert raw(lib, 'kge_gather_rows', d_X, ld, d_idx, idx.shape[0], K, got['gather']) == 0, tag
        d_N = carve(X, pad, o, NAN, device='cuda')
        assert raw(lib, 'kge_normalize_rows', d_N, ld, rows, K) == 0, tag
        d_F = carve(X * 3, pad, o, NAN, device='cuda')
        assert raw(lib, 'kge_frac_rows', d_F, ld, rows, K) == 0, tag
        got['norm'], got['frac'] = d_N, d_F
        torch.cuda.synchronize()
        for name, t in got.items():
            assert bool(torch.isfinite(t).all()), (tag, name, 'poison reached the output')
            assert_guard_intact(t)
        for v in (d_X, d_Y, d_idx, mx):
            assert_guard_intact(v)
        assert np.array_equal(got['sq'].cpu().numpy(), n_ref), tag
        assert np.array_equal(got['dot'].cpu().numpy(), d_ref) and np.array_equal(got['dot_yx'].cpu().numpy(), d_ref), tag
        a = got['any'].cpu().numpy().astype(np.float64)
        assert (np.abs(a - n64) / np.maximum(n64, 1e-30)).max() < 1e-6, tag         # (the any-order test's tolerance)
        assert float(mx[0]) == float(n_ref.max()) and float(mx[1]) == float(got['any'].max()), tag
        assert np.array_equal(got['gather'].cpu().numpy(), X[idx].numpy()), tag
        assert np.abs(got['norm'].cpu().numpy() - norm64).max() < TOL, tag
        assert np.array_equal(got['frac'].cpu().numpy(), frac_ref), tag
        if not base:
            base = {k: v.clone() for k, v in got.items()}
        for name in got:
            if name == 'any':       # no bit contract: the summation order may depend on the body taken
                continue
            assert same_bits(got[name], base[name]), (tag, name)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1025])
def test_ewise_and_absmax_at_element_offsets(hip, n):
    """kge_ewise (every op) and kge_absmax on vectors 0..3 floats off a 16-byte boundary: separate mul / add roundings
    (torch's own on the CPU), NaN around the operands, sentinel around the output."""
    lib = hip.load_library()
    g = torch.Generator().manual_seed(n)
    a, b, c, d = [rnd(g, n) for _ in range(4)]
    refs = [a + b, a - b, a * b, a * b - c * d, a * b + c * d]
    for oa in range(4):
        for ob in ((oa,) if n > 5 else range(4)):
            d_a, d_b = carve(a, off=oa, device='cuda'), carve(b, off=ob, device='cuda')
            d_c, d_d = carve(c, off=(oa + 1) % 4, device='cuda'), carve(d, off=(ob + 3) % 4, device='cuda')
            for op, ref in enumerate(refs):
                out = guarded_out(n, off=(oa + ob + op) % 4)
                assert raw(lib, 'kge_ewise', op, d_a, d_b, d_c if op >= 3 else None, d_d if op >= 3 else None, n, out) == 0
                torch.cuda.synchronize()
                assert same_bits(out.cpu(), ref), (oa, ob, op)
                assert_guard_intact(out)
            mx = guarded_out(1, off=ob)
            mx.zero_()
            assert raw(lib, 'kge_absmax', d_a, n, mx) == 0
            torch.cuda.synchronize()
            assert float(mx[0]) == float(a.abs().max())
            for v in (d_a, d_b, d_c, d_d, mx):
                assert_guard_intact(v)


# ---------------------------------------------------------------------------
# C. operand builders of the prefilters
# ---------------------------------------------------------------------------
def _near(a, b):
    """Side outputs that only bound an error (cell sums, residual norms): equal up to the summation order."""
    a, b = a.double().cpu(), b.double().cpu()
    return a.shape == b.shape and bool(((a - b).abs() <= 1e-5 * b.abs() + 1e-30).all())


@pytest.mark.parametrize('rows,K', [(33, 17), (193, 17), (257, 64), (65, 8), (5, 1), (129, 203), (64, 200), (31, 4)])
def test_prefilter_operand_builders_on_carved_input(hip, rows, K):
    """kge_lp_split_rows, kge_lp_hi_rows, kge_lp_hi_rows_frag, kge_lp_sad_rows and kge_lp_dot_table_prep on carved input
    (queries and candidates, L2 and two-segment DOT conventions, row_index gathers): the operand bytes equal, byte for
    byte, those built from the packed copy; nothing outside the operands is written."""
    lib = hip.load_library()
    g = torch.Generator().manual_seed(rows * 31 + K)
    X0 = torch.nn.functional.normalize(torch.randn(rows, K, generator=g), dim=1) * 1.2
    X1 = torch.nn.functional.normalize(torch.randn(rows, K, generator=g), dim=1) * 0.7
    aug = (X0 ** 2).sum(1) + (X1 ** 2).sum(1)
    idx = torch.cat([torch.tensor([0, rows - 1, rows - 1]), torch.randint(0, rows, (rows + 4,), generator=g)])
    nmax = torch.tensor([float((X0 ** 2).sum(1).max()), float((X1 ** 2).sum(1).max())]).cuda()
    bounds = torch.tensor([float(torch.cat([X0, X1]).abs().max()), 0.25]).cuda()      # emax, rmax of the SAD operands
    f = ctypes.c_float

    def build(d0, d1, d_aug, d_idx):
        ld0, ld1 = d0.stride(0), d1.stride(0)
        exact, soft, guards = {}, {}, []
        for is_query in (0, 1):
            for dot in (False, True):
                for gather in ((False, True) if is_query else (False,)):
                    key = (is_query, dot, gather)
                    n_out = idx.shape[0] if gather else rows
                    K1 = K if dot else 0
                    if dot:
                        aug_mode, aug_mul = (3, 1.0) if is_query else (4, 0.0)
                    else:
                        aug_mode, aug_mul = (2, 1.0) if is_query else (1, -0.5)
                    a_ptr = d_aug if aug_mode in (1, 3) else None
                    n0, n1 = (nmax[0:1], nmax[1:2]) if dot else (None, None)
                    rows_p = int(lib.kge_lp_split_rows_padded(n_out, is_query))
                    units = int(lib.kge_lp_split_units(K + K1, 1))
                    out, css = guarded_out(rows_p * units * 64, dtype=torch.uint8), guarded_out(units * rows_p)
                    assert raw(lib, 'kge_lp_split_rows', d0, ld0, K, d1 if dot else None, ld1 if dot else 0, K1, n_out, is_query,
                               aug_mode, a_ptr, f(aug_mul), n0, n1, out, css, d_idx if gather else None) == 0, key
                    exact[('split',) + key], soft[('css',) + key] = out, css
                    hunits = int(lib.kge_lp_hi_units(K + K1))
                    out, dn2, dmx = guarded_out(rows_p * hunits * 32, dtype=torch.uint8), guarded_out(n_out, off=1), guarded_out(1)
                    dmx.zero_()
                    assert raw(lib, 'kge_lp_hi_rows', d0, ld0, K, d1 if dot else None, ld1 if dot else 0, K1, n_out, is_query,
                               aug_mode, a_ptr, f(aug_mul), n0, n1, out, dn2, dmx, d_idx if gather else None) == 0, key
                    exact[('hi',) + key], soft[('dn2',) + key], soft[('dmx',) + key] = out, dn2, dmx
                    if not is_query:
                        out, dn2, dmx = guarded_out(rows_p * hunits * 32, dtype=torch.uint8), guarded_out(rows, off=3), guarded_out(1)
                        dmx.zero_()
                        assert raw(lib, 'kge_lp_hi_rows_frag', d0, ld0, K, d1 if dot else None, ld1 if dot else 0, K1, rows,
                                   aug_mode, a_ptr, f(aug_mul), n0, n1, out, dn2, dmx) == 0, key
                        exact[('frag',) + key], soft[('fdn2',) + key], soft[('fdmx',) + key] = out, dn2, dmx
        Kp = int(lib.kge_lp_sad_cols_padded(K))
        for gather in (False, True):
            n_out = idx.shape[0] if gather else rows
            out = guarded_out(n_out, Kp, 0, 0, dtype=torch.int16)
            assert raw(lib, 'kge_lp_sad_rows', d0, ld0, n_out, K, bounds[0:1], bounds[1:2], out, d_idx if gather else None) == 0
            exact[('sad', gather)] = out
        rows_p, hunits = int(lib.kge_lp_split_rows_padded(rows, 0)), int(lib.kge_lp_hi_units(2 * K))
        for frag in (0, 1):
            out, dnb = guarded_out(rows_p * hunits * 32, dtype=torch.uint8), guarded_out(int(lib.kge_lp_dot_table_prep_blocks(rows, 1)))
            ws, nm = guarded_out(2 * int(lib.kge_lp_dot_table_prep_blocks(rows, 0))), guarded_out(2, off=2)
            nm.zero_()
            assert raw(lib, 'kge_lp_dot_table_prep', d0, ld0, K, d1, ld1, K, rows, frag, nm[0:1], nm[1:2], out, dnb, ws) == 0
            exact[('dot_table', frag)], soft[('dot_nm', frag)] = out, nm
            guards += [dnb, ws]
        torch.cuda.synchronize()
        for v in list(exact.values()) + list(soft.values()) + guards + [d0, d1, d_aug, d_idx]:
            assert_guard_intact(v)
        return exact, soft
    base_exact, base_soft = build(carve(X0, 0, 0, device='cuda'), carve(X1, 0, 0, device='cuda'), carve(aug, device='cuda'),
                                  carve(idx, poison=rows, device='cuda'))
    for v in base_soft.values():
        assert bool(torch.isfinite(v).all())
    lays = ROW_LAYOUTS if rows in (33, 65) else FEW
    for pad, o in lays:
        for p0, o0, p1, o1 in ((pad, o, pad, o), (pad, o, 0, 0), (0, 0, pad, o)):
            tag = 'X0 %d.%d X1 %d.%d' % (p0, o0, p1, o1)
            exact, soft = build(carve(X0, p0, o0, device='cuda'), carve(X1, p1, o1, device='cuda'), carve(aug, off=o, device='cuda'),
                                carve(idx, off=o % 2, poison=rows, device='cuda'))
            for k, v in exact.items():
                assert torch.equal(bits8(v), bits8(base_exact[k])), (tag, k)
            for k, v in soft.items():
                assert bool(torch.isfinite(v).all()) and _near(v, base_soft[k]), (tag, k)


def bits8(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize('B,N,K', [(193, 257, 17), (700, 1500, 203), (130, 300, 64)])
def test_prefilter_counts_with_a_carved_exact_score_descriptor(hip, B, N, K):
    """kge_lp_split_count + kge_lp_split_recheck (TransE-L2) and kge_lp_sad_count + kge_lp_sad_recheck (TransE-L1) with the
    exact-score descriptor -- what the recheck re-scores the uncertain pairs with -- carved: raw_count is what
    kge_lp_count_ge leaves for the packed problem (shapes of test_split_prefilter_counts_equal_exact_counts)."""
    lib = hip.load_library()
    g = torch.Generator().manual_seed(B + N)
    E = torch.nn.functional.normalize(torch.randn(N, K, generator=g), dim=1)
    R = torch.nn.functional.normalize(torch.randn(9, K, generator=g), dim=1)
    h, r, t = [torch.randint(0, n, (B,), generator=g) for n in (N, 9, N)]
    E[N // 2] = E[0]                                   # exact duplicates: ties with the true entity
    Q = E[h] + R[r]
    lays = [(0, 0), (3, 1), (4, 2), (8, 0), (0, 3), (1, 0)]
    # --- L2: f16 hi/lo split prefilter
    want = None
    for pad, o in lays:
        dQ, dE = carve(Q, pad, o, device='cuda'), carve(E, pad, (o + 1) % 4 if pad == 0 and o else o, device='cuda')
        guard = guarded_out(4, off=o)
        guard.zero_()
        qn, en = guarded_out(B, off=o), guarded_out(N, off=(o + 2) % 4)
        assert raw(lib, 'kge_row_sqnorm', dQ, dQ.stride(0), B, K, qn, guard[0:1]) == 0
        assert raw(lib, 'kge_row_sqnorm', dE, dE.stride(0), N, K, en, guard[1:2]) == 0
        prob = hip.LpProblem(hip.LP_L2_EXPAND, dQ, dE, qn=qn, en=en)
        d_t = carve(t, off=o % 2, poison=N, device='cuda')
        st = guarded_out(B, off=(o + 1) % 4)
        assert raw(lib, 'kge_lp_pair_scores', prob.desc, None, d_t, B, st) == 0
        exact = prob.count_ge(st)
        if want is None:
            want, st0 = exact.clone(), st.clone()
        assert torch.equal(exact, want) and same_bits(st, st0), (pad, o)
        Es, e2 = hip.split_table(dE, aug=en)
        prob.split = {'Es': Es, 'e2pref': e2, 'enmax': guard[1:2], 'overflow': guard[2:3]}
        got = prob.count_ge(st)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (pad, o, int((got != want).sum()))
        assert float(guard[2]) == 0.0 and B <= int(prob.last_split[0].item()) <= 64 * B
        for v in (dQ, dE, guard, qn, en, st, d_t):
            assert_guard_intact(v)
    # --- L1: 16-bit SAD prefilter
    E1, Q1 = rnd(g, N, K) * 0.3, rnd(g, B, K) * 0.45         # (the operands of test_l1_sad_prefilter_counts_equal_exact_counts)
    E1[5] = E1[3]
    want = None
    for pad, o in lays:
        dQ, dE = carve(Q1, pad, o, device='cuda'), carve(E1, pad, o, device='cuda')
        prob = hip.LpProblem(hip.LP_L1_DIRECT, dQ, dE)
        d_t = carve(t, off=(o + 1) % 2, poison=N, device='cuda')
        st = guarded_out(B, off=o)
        assert raw(lib, 'kge_lp_pair_scores', prob.desc, None, d_t, B, st) == 0
        exact = prob.count_ge(st)
        if want is None:
            want = exact.clone()
        assert torch.equal(exact, want), (pad, o)
        bounds = guarded_out(3, off=(o + 3) % 4)
        bounds.zero_()
        hip.absmax(torch.cat([Q1.reshape(-1), E1.reshape(-1)]).cuda(), bounds[0:1])     # rmax = 0: the bound is max |x| itself
        prob.sad = {'Ei': hip.sad_rows(dE, bounds[0:1], bounds[1:2]), 'emax': bounds[0:1], 'rmax': bounds[1:2],
                    'overflow': bounds[2:3]}
        got = prob.count_ge(st)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (pad, o, int((got != want).sum()))
        assert float(bounds[2]) == 0.0 and int(prob.last_split[0]) <= max(64, 0.05 * B * N)
        for v in (dQ, dE, st, d_t, bounds):
            assert_guard_intact(v)


# ---------------------------------------------------------------------------
# D. fused entry points that refuse unaligned input
# ---------------------------------------------------------------------------
def w_rows(W, r_idx, k):
    return W[r_idx][:, :k].numpy()


def test_proj_query_stats_refuses_and_the_separate_kernels_give_its_bits(hip):
    """kge_proj_query_stats: KGE_EUNSUPPORTED for K % 4, ldq % 4, ldw % 4 and a base 4 bytes off, one violated
    precondition at a time; no output is touched; kge_row_sqnorm / kge_gather_rows / kge_row_dot on the SAME unaligned
    operands then give the bits the fused launch gives on packed copies (what _hip.proj_query_stats' callers do)."""
    lib = hip.load_library()
    rows, K, R = 77, 24, 6
    g = torch.Generator().manual_seed(5)
    Q, W = rnd(g, rows, K), rnd(g, R, K)
    r_idx = torch.randint(0, R, (rows,), generator=g)
    scale, z_add = 2.0, -2.0
    d_r = carve(r_idx, off=1, poison=R, device='cuda')
    qn0, pz0, qm0 = guarded_out(rows), guarded_out(rows, 2), guarded_out(1, off=1)
    qm0.zero_()
    d_Q, d_W = carve(Q, 0, 0, device='cuda'), carve(W, 0, 0, device='cuda')
    assert raw(lib, 'kge_proj_query_stats', d_Q, K, d_W, K, d_r, rows, K, ctypes.c_float(scale), ctypes.c_float(z_add), qn0,
               pz0, qm0, None, 0) == 0
    torch.cuda.synchronize()
    for v in (qn0, pz0, qm0, d_Q, d_W):
        assert_guard_intact(v)
    got = hip.proj_query_stats(d_Q, d_W, d_r, scale, z_add)       # the wrapper, on aligned input: the fused path
    assert got is not None and same_bits(got[0], qn0) and same_bits(got[1], pz0)
    cases = {'K % 4': (Q[:, :K - 1], W[:, :K - 1], (0, 0), (0, 0)), 'ldq % 4': (Q, W, (1, 0), (0, 0)),
             'ldw % 4': (Q, W, (0, 0), (3, 0)), 'Q base': (Q, W, (0, 1), (0, 0)), 'W base': (Q, W, (4, 0), (8, 3)),
             'both': (Q, W, (3, 2), (1, 1))}
    for name, (q, w, (qp, qo), (wp, wo)) in cases.items():
        k = q.shape[1]
        d_Q, d_W = carve(q, qp, qo, device='cuda'), carve(w, wp, wo, device='cuda')
        qn, pz, qm = guarded_out(rows, off=1), guarded_out(rows, 2, 0, 2), guarded_out(1)
        zero = guarded_out(9, dtype=torch.int32)
        rc = raw(lib, 'kge_proj_query_stats', d_Q, k + qp, d_W, k + wp, d_r, rows, k, ctypes.c_float(scale),
                 ctypes.c_float(z_add), qn, pz, qm, zero, 9)
        assert rc == KGE_EUNSUPPORTED, (name, rc)
        torch.cuda.synchronize()
        for v in (qn, pz, qm, zero):
            assert_guard_intact(v, rows=0)      # nothing was launched: not one element written
        # the fallback: the separate chains on the same unaligned operands
        f_qn, f_uw, f_ww = guarded_out(rows), guarded_out(rows), guarded_out(rows)
        Wr = guarded_out(rows, k, qp, qo)       # gathered W rows, laid out like Q (kge_row_dot has ONE ld)
        Wp = guarded_out(rows * (k + qp))
        assert raw(lib, 'kge_row_sqnorm', d_Q, k + qp, rows, k, f_qn, None) == 0
        assert raw(lib, 'kge_gather_rows', d_W, k + wp, d_r, rows, k, Wp) == 0          # (packed rows of length k)
        Wr.copy_(Wp[:rows * k].view(rows, k))
        assert raw(lib, 'kge_row_dot', d_Q, Wr, k + qp, rows, k, ctypes.c_float(scale), f_uw) == 0
        assert raw(lib, 'kge_row_sqnorm', Wr, k + qp, rows, k, f_ww, None) == 0
        torch.cuda.synchronize()
        w = hip.proj_query_stats(d_Q, d_W, d_r, scale, z_add)         # the wrapper packs a strided view before the call
        if name == 'K % 4' or d_Q.is_contiguous() and d_W.is_contiguous():
            assert w is None, name          # refused: its callers run the separate kernels
        else:
            assert w is not None and same_bits(w[0], qn0) and same_bits(w[1], pz0), name
        if name != 'K % 4':
            assert same_bits(f_qn, qn0) and same_bits(f_uw, pz0[:, 0]) and same_bits(f_ww + z_add, pz0[:, 1]), name
        else:                               # K = 23: the chains of the oracle on the packed columns
            orc_c = oracle_clib()
            qp, wp = np.ascontiguousarray(q.numpy()), np.ascontiguousarray(w_rows(W, r_idx, k))
            r_qn, r_uw, r_ww = np.empty(rows, np.float32), np.empty(rows, np.float32), np.empty(rows, np.float32)
            orc_c.orc_row_sqnorm_chain(fptr(qp), i64(k), i64(rows), i64(k), fptr(r_qn))
            orc_c.orc_row_sqnorm_chain(fptr(wp), i64(k), i64(rows), i64(k), fptr(r_ww))
            orc_c.orc_row_dot_chain(fptr(qp), i64(k), fptr(wp), i64(k), i64(rows), i64(k), ctypes.c_float(scale), fptr(r_uw))
            assert np.array_equal(f_qn.cpu().numpy(), r_qn) and np.array_equal(f_uw.cpu().numpy(), r_uw), name
            assert np.array_equal(f_ww.cpu().numpy(), r_ww), name
        for v in (f_qn, f_uw, f_ww, Wp, d_Q, d_W):
            assert_guard_intact(v)


def test_table_prep_l2_refuses_and_the_separate_kernels_give_its_bits(hip):
    """kge_lp_table_prep_l2: KGE_EUNSUPPORTED for K % 4, ld % 4 and a base 4 bytes off; en / out / the maxima untouched;
    kge_row_sqnorm + kge_lp_hi_rows_frag on the unaligned table give the fused pass's bits (en: bit for bit, the hi table
    byte for byte)."""
    lib = hip.load_library()
    N, K = 300, 40
    g = torch.Generator().manual_seed(9)
    E = torch.nn.functional.normalize(torch.randn(N, K, generator=g), dim=1) * 1.3
    units_p, rows_p = int(lib.kge_lp_hi_units(K)), int(lib.kge_lp_split_rows_padded(N, 0))
    nbytes = rows_p * units_p * 32

    def fused(d_E, ld, k):
        en, out, mx = guarded_out(N, off=1), guarded_out(nbytes, dtype=torch.uint8), guarded_out(2)
        mx.zero_()
        rc = raw(lib, 'kge_lp_table_prep_l2', d_E, ld, N, k, en, mx[0:1], out, mx[1:2], None)
        torch.cuda.synchronize()
        return rc, en, out, mx
    d_E = carve(E, 0, 0, device='cuda')
    rc, en0, out0, mx0 = fused(d_E, K, K)
    assert rc == 0
    for v in (en0, out0, mx0, d_E):
        assert_guard_intact(v)
    w = hip.table_prep_l2(d_E, torch.zeros(1, device='cuda'), torch.zeros(1, device='cuda'))
    assert w is not None and same_bits(w[0], en0) and torch.equal(w[1], out0)
    for name, (e, pad, off) in {'K % 4': (E[:, :K - 1], 1, 0), 'ld % 4': (E, 3, 0), 'base': (E, 0, 1)}.items():
        k = e.shape[1]
        d_E = carve(e, pad, off, device='cuda')
        rc, en, out, mx = fused(d_E, k + pad, k)
        assert rc == KGE_EUNSUPPORTED, (name, rc)
        assert_guard_intact(en, rows=0)
        assert_guard_intact(out, rows=0)
        assert float(mx[0]) == 0.0 and float(mx[1]) == 0.0
        w = hip.table_prep_l2(d_E, mx[0:1], mx[1:2])
        if name == 'ld % 4':        # the wrapper packs the strided view: the fused pass, the packed table's bits
            assert w is not None and same_bits(w[0], en0) and torch.equal(w[1], out0), name
        else:
            assert w is None, name  # refused: its callers run the separate kernels
        if name == 'K % 4':
            continue
        f_en, f_out, dn = guarded_out(N, off=2), guarded_out(nbytes, dtype=torch.uint8), guarded_out(1)
        dn.zero_()
        assert raw(lib, 'kge_row_sqnorm', d_E, k + pad, N, k, f_en, None) == 0
        assert raw(lib, 'kge_lp_hi_rows_frag', d_E, k + pad, k, None, 0, 0, N, 1, f_en, ctypes.c_float(-0.5), None, None, f_out,
                   None, dn) == 0
        torch.cuda.synchronize()
        assert same_bits(f_en, en0) and torch.equal(f_out, out0), name
        assert abs(float(dn[0]) - float(mx0[1])) <= 3e-4 * float(mx0[1]) + 1e-30    # (a bound: test_table_prep_l2_equals_...)
        for v in (f_en, f_out, dn, d_E):
            assert_guard_intact(v)


def test_dot_table_prep_fused_refuses_unreadable_rows(hip):
    """kge_lp_dot_table_prep_fused: KGE_EINVAL unless the rows are float4-readable (K0, K1, ld0, ld1 % 4 == 0, 16-byte
    aligned bases), one violation at a time; the outputs stay untouched; kge_lp_dot_table_prep (the two-launch form, which
    takes any layout) builds from the unaligned tables the bytes it builds from packed copies."""
    lib = hip.load_library()
    N, K = 200, 24
    g = torch.Generator().manual_seed(11)
    X0, X1 = rnd(g, N, K), rnd(g, N, K)
    units_p, rows_p = int(lib.kge_lp_hi_units(2 * K)), int(lib.kge_lp_split_rows_padded(N, 0))
    nbytes = rows_p * units_p * 32
    nb = int(lib.kge_lp_dot_table_prep_blocks(N, 1))
    nb0 = int(lib.kge_lp_dot_table_prep_blocks(N, 0))
    prev = torch.full((2,), 64.0, device='cuda')

    def two_launch(d0, ld0, k0, d1, ld1, k1):
        out, dnb, ws = guarded_out(nbytes, dtype=torch.uint8), guarded_out(nb), guarded_out(2 * nb0)
        nm = guarded_out(2, off=1)
        nm.zero_()
        rc = raw(lib, 'kge_lp_dot_table_prep', d0, ld0, k0, d1, ld1, k1, N, 1, nm[0:1], nm[1:2], out, dnb, ws)
        torch.cuda.synchronize()
        assert rc == 0
        for v in (out, dnb, ws, nm):
            assert_guard_intact(v)
        return out, nm
    p0, p1 = carve(X0, 0, 0, device='cuda'), carve(X1, 0, 0, device='cuda')
    out_ref, nm_ref = two_launch(p0, K, K, p1, K, K)
    out, dnb, nmb = guarded_out(nbytes, dtype=torch.uint8), guarded_out(nb), guarded_out(2 * nb)
    assert raw(lib, 'kge_lp_dot_table_prep_fused', p0, K, K, p1, K, K, N, prev, out, dnb, nmb) == 0
    torch.cuda.synchronize()
    for v in (out, dnb, nmb, p0, p1):
        assert_guard_intact(v)
    assert bool(torch.isfinite(nmb).all()) and bool(torch.isfinite(dnb).all())
    cases = {'K0 % 4': (X0[:, :K - 1], 1, 0, X1, 0, 0), 'K1 % 4': (X0, 0, 0, X1[:, :K - 2], 2, 0), 'ld0 % 4': (X0, 1, 0, X1, 0, 0),
             'ld1 % 4': (X0, 0, 0, X1, 3, 0), 'X0 base': (X0, 0, 1, X1, 0, 0), 'X1 base': (X0, 4, 0, X1, 8, 3)}
    for name, (a, pa, oa, b, pb, ob) in cases.items():
        d0, d1 = carve(a, pa, oa, device='cuda'), carve(b, pb, ob, device='cuda')
        out, dnb, nmb = guarded_out(nbytes, dtype=torch.uint8), guarded_out(nb), guarded_out(2 * nb)
        rc = raw(lib, 'kge_lp_dot_table_prep_fused', d0, a.shape[1] + pa, a.shape[1], d1, b.shape[1] + pb, b.shape[1], N, prev,
                 out, dnb, nmb)
        assert rc == KGE_EINVAL, (name, rc)
        torch.cuda.synchronize()
        for v in (out, dnb, nmb):
            assert_guard_intact(v, rows=0)
        assert hip.dot_table_prep_fusable(d0, d1) is False, name
        if a.shape[1] == K and b.shape[1] == K:
            got, nm = two_launch(d0, K + pa, K, d1, K + pb, K)
            # (the maxima only fix a power-of-two scale: any summation order, compared to rounding)
            assert torch.equal(got, out_ref) and bool(((nm - nm_ref).abs() <= 1e-6 * nm_ref).all()), name
            nmw = torch.zeros(2, device='cuda')         # the wrapper (it packs strided views): the same table bytes
            assert torch.equal(hip.dot_table_prep(d0, d1, nmw[0:1], nmw[1:2], True)[0], out_ref), name
        assert_guard_intact(d0)
        assert_guard_intact(d1)


def test_count_ge_cols_refuses_what_the_packed_fma_kernel_cannot_read(hip):
    """kge_lp_count_ge_cols: KGE_EINVAL for anything but a plain KGE_LP_L2_DIRECT problem with K0 % 4 == 0, lda0 / ldt0
    % 4 == 0 and 16-byte aligned A0 / T0 (one violation at a time, the counters untouched); on aligned operands its
    counts are those of kge_lp_count_ge, which takes every layout."""
    lib = hip.load_library()
    B, N, K = 70, 300, 24
    ops = make_ops('l2d', B, N, K)
    S = packed_scores(hip, 'l2d', ops).cpu().numpy()
    g = torch.Generator().manual_seed(3)
    st = S[np.arange(B), torch.randint(0, N, (B,), generator=g).numpy()]
    cnt_ref = (S >= st[:, None]).sum(1).astype(np.int32)
    Bp = B                                  # one column per query: column r is query row rep[r] = r, compared by col_q[r] = r
    rep = torch.arange(Bp)
    col_q = torch.arange(B).to(torch.int32)
    d_rep, d_col = carve(rep, off=1, poison=0, device='cuda'), carve(col_q, off=3, poison=-1, device='cuda')
    d_st = carve(torch.from_numpy(st.copy()), off=1, device='cuda')

    def run(mode, o, lay):
        prob, dv = problem(hip, mode, o, lay)
        cnt = guarded_out(B, off=2, dtype=torch.int32)
        cnt.zero_()
        rc = raw(lib, 'kge_lp_count_ge_cols', prob.desc, d_st, cnt, d_rep, d_col, Bp, None, 0)
        torch.cuda.synchronize()
        assert_guard_intact(cnt)
        return rc, cnt, prob
    for lay in ({}, {'A0': (4, 0), 'T0': (8, 0)}):
        rc, cnt, prob = run('l2d', ops, lay)
        assert rc == 0 and np.array_equal(cnt.cpu().numpy(), cnt_ref), lay
    ops3 = {'A0': ops['A0'][:, :K - 1], 'T0': ops['T0'][:, :K - 1]}
    refused = {'K0 % 4': ('l2d', ops3, {'A0': (1, 0), 'T0': (1, 0)}), 'lda0 % 4': ('l2d', ops, {'A0': (1, 0)}),
               'ldt0 % 4': ('l2d', ops, {'T0': (3, 0)}), 'A0 base': ('l2d', ops, {'A0': (0, 1)}),
               'T0 base': ('l2d', ops, {'T0': (4, 3)}), 'L1': ('l1d', ops, {}), 'rank-1 term': ('l2d_ax', make_ops('l2d_ax', B, N, K), {})}
    for name, (mode, o, lay) in refused.items():
        rc, cnt, prob = run(mode, o, lay)
        assert rc == KGE_EINVAL, (name, rc)
        assert int(cnt.abs().sum()) == 0, name          # still the caller's zeros: nothing was launched
        if o is ops and mode == 'l2d':                  # the general kernel takes the same descriptor
            assert raw(lib, 'kge_lp_count_ge', prob.desc, d_st, cnt) == 0
            torch.cuda.synchronize()
            assert np.array_equal(cnt.cpu().numpy(), cnt_ref), name
            assert_guard_intact(cnt)


def _pipeline_tables(g, n_ent, n_rel, d):
    E = torch.nn.functional.normalize(torch.randn(n_ent, d, generator=g), dim=1)
    R = torch.randn(n_rel, d, generator=g) * 0.1
    return E, R


def test_query_pipeline_refuses_unaligned_tables(hip):
    """kge_lp_query_pipeline (TransE-L2, contiguous tables: the layout axis is the base): KGE_EINVAL for d % 4 != 0 or a
    table 4 bytes off a 16-byte boundary, every output untouched; kge_lp_prep + kge_row_sqnorm on the same unaligned tables
    give the Q and qn the fused launch gives on aligned copies."""
    lib = hip.load_library()
    n_ent, n_rel, d, B = 300, 7, 24, 50
    g = torch.Generator().manual_seed(21)
    E, R = _pipeline_tables(g, n_ent, n_rel, d)
    h, t, r = [torch.randint(0, n, (B,), generator=g) for n in (n_ent, n_ent, n_rel)]
    d_h, d_t, d_r = [carve(x, off=1, poison=0, device='cuda') for x in (h, t, r)]
    Bp = int(lib.kge_lp_split_rows_padded(B, 1))

    def fused(d_E, d_R, dd):
        units_p = int(lib.kge_lp_split_units(dd, 1))
        en = hip.row_sqnorm(d_E.contiguous())
        emax = en.max().view(1).clone()
        o = {'Q': guarded_out(B, dd), 'qn': guarded_out(B, off=1), 's_true': guarded_out(B, off=2),
             'Qs': guarded_out(Bp * units_p * 64, dtype=torch.uint8), 'thr': guarded_out(4 * Bp), 'n_list': guarded_out(1, dtype=torch.int32),
             'qmax': guarded_out(1, off=3), 'zero': guarded_out(5, dtype=torch.int32)}
        o['qmax'].zero_()
        rc = raw(lib, 'kge_lp_query_pipeline', hip.SIDE_TAIL, d_E, d_R, dd, d_h, d_t, d_r, B, en, emax, o['qmax'],
                 hip.split_accum_model(), ctypes.c_float(1.0), o['Q'], o['qn'], o['s_true'], o['Qs'], o['thr'], o['n_list'], None,
                 None, 0, None, None, None, 0, o['zero'], 5)
        torch.cuda.synchronize()
        return rc, o
    rc, ok = fused(carve(E, 0, 0, device='cuda'), carve(R, 0, 0, device='cuda'), d)
    assert rc == 0
    for v in ok.values():
        assert_guard_intact(v)
    assert int(ok['zero'].abs().sum()) == 0
    for name, (e, rr, oe, orr) in {'d % 4': (E[:, :d - 1], R[:, :d - 1], 0, 0), 'E base': (E, R, 1, 0), 'R base': (E, R, 0, 3)}.items():
        dd = e.shape[1]
        d_E, d_R = carve(e, 0, oe, device='cuda'), carve(rr, 0, orr, device='cuda')
        rc, o = fused(d_E, d_R, dd)
        assert rc == KGE_EINVAL, (name, rc)
        assert float(o['qmax'][0]) == 0.0
        for k, v in o.items():
            assert_guard_intact(v, rows=1 if k == 'qmax' else 0)
        if dd == d:     # the separate kernels on the unaligned tables: the fused launch's Q / qn bits
            Q0, _, qn, _ = hip.lp_prep(hip.TRANSE_L2, hip.SIDE_TAIL, [d_E, d_R], d, d, d_h, d_t, d_r, want_qn=True)
            assert same_bits(Q0, ok['Q']) and same_bits(qn, ok['qn']), name
            en_u = hip.row_sqnorm(d_E)
            st_u = hip.LpProblem(hip.LP_L2_EXPAND, Q0, d_E, qn=qn, en=en_u).pair_scores(d_t)
            assert same_bits(st_u, ok['s_true']), name
        assert_guard_intact(d_E)
        assert_guard_intact(d_R)


def test_dot_query_pipeline_refuses_unaligned_tables(hip):
    """kge_lp_dot_query_pipeline (DistMult here): KGE_EINVAL unless d % 8 == 0 and the tables are 16-byte aligned, every
    output untouched; kge_lp_prep on the same unaligned tables gives the Q0 the fused launch gives on aligned copies."""
    lib = hip.load_library()
    n_ent, n_rel, d, B = 300, 7, 24, 50
    g = torch.Generator().manual_seed(22)
    E, R = _pipeline_tables(g, n_ent, n_rel, d)
    h, t, r = [torch.randint(0, n, (B,), generator=g) for n in (n_ent, n_ent, n_rel)]
    d_h, d_t, d_r = [carve(x, off=1, poison=0, device='cuda') for x in (h, t, r)]
    Bp = int(lib.kge_lp_split_rows_padded(B, 1))
    scal = torch.tensor([4.0, 1e-6], device='cuda')         # emax0, de2max: device scalars of the candidate table

    def fused(d_E, d_R, dd):
        units_p = int(lib.kge_lp_hi_units(dd))
        o = {'Q': guarded_out(B, dd), 'qn': guarded_out(B, off=1), 's_true': guarded_out(B, off=2),
             'Qh': guarded_out(Bp * units_p * 32, dtype=torch.uint8), 'thr': guarded_out(4 * Bp), 'q_dn2': guarded_out(B, off=3),
             'n_list': guarded_out(1, dtype=torch.int32), 'overflow': guarded_out(1), 'qmax': guarded_out(1, off=3),
             'zero': guarded_out(5, dtype=torch.int32)}
        o['qmax'].zero_()
        o['overflow'].zero_()
        rc = raw(lib, 'kge_lp_dot_query_pipeline', hip.SIDE_TAIL, d_E, None, d_R, None, dd, d_h, d_t, d_r, B, scal[0:1], None,
                 scal[1:2], o['qmax'], hip.split_accum_model(), ctypes.c_float(1.0), o['Q'], None, o['qn'], o['s_true'], o['Qh'],
                 o['thr'], o['q_dn2'], o['n_list'], o['overflow'], o['zero'], 5, None, 0, None, 0, None)
        torch.cuda.synchronize()
        return rc, o
    rc, ok = fused(carve(E, 0, 0, device='cuda'), carve(R, 0, 0, device='cuda'), d)
    assert rc == 0
    for v in ok.values():
        assert_guard_intact(v)
    for name, (e, rr, oe, orr) in {'d % 8': (E[:, :d - 4], R[:, :d - 4], 0, 0), 'd % 4': (E[:, :d - 1], R[:, :d - 1], 0, 0),
                                   'E base': (E, R, 1, 0), 'R base': (E, R, 0, 3)}.items():
        dd = e.shape[1]
        d_E, d_R = carve(e, 0, oe, device='cuda'), carve(rr, 0, orr, device='cuda')
        rc, o = fused(d_E, d_R, dd)
        assert rc == KGE_EINVAL, (name, rc)
        for k, v in o.items():
            assert_guard_intact(v, rows=1 if k in ('qmax', 'overflow') else 0)
        assert float(o['qmax'][0]) == 0.0 and float(o['overflow'][0]) == 0.0
        if dd == d:
            Q0 = hip.lp_prep(hip.DISTMULT, hip.SIDE_TAIL, [d_E, d_R], d, d, d_h, d_t, d_r)[0]
            assert same_bits(Q0, ok['Q']), name
            assert same_bits(hip.LpProblem(hip.LP_DOT, Q0, d_E).pair_scores(d_t), ok['s_true']), name
        assert_guard_intact(d_E)
        assert_guard_intact(d_R)


# ---------------------------------------------------------------------------
# E. fused gather + normalise + score, its backward and the gradient reductions
# ---------------------------------------------------------------------------
TRIPLE_KINDS = ['transe_l1', 'transe_l2', 'transh', 'transd', 'distmult', 'complex', 'rescal', 'hole', 'toruse_l1',
                'toruse_tl1', 'toruse_tl2', 'toruse_tel2', 'transr']          # index = the KGE_* kind code of the header
N_STREAMS = {'transh': 4, 'complex': 6, 'transd': 6, 'rescal': 4, 'transr': 4}   # gradient-row streams (default 3)
TORUS_DISS = {'toruse_l1': 'L1', 'toruse_tl1': 'torus_L1', 'toruse_tl2': 'torus_L2', 'toruse_tel2': 'torus_eL2'}
GRAD_TOL = 1e-4     # the backward tests' bound: |got - want| <= 1e-4 * max(1, max |want|)


def triple_tables(kind, d, g, n_ent=40, n_rel=6):
    """(tables, d_ent, d_rel) of one model kind; TransD and TransR get d_rel != d_ent."""
    def T(n, k, s=0.5):
        return torch.randn(n, k, generator=g) * s
    if kind == 'transd':
        dr = max(1, d - d // 3)
        return [T(n_ent, d), T(n_rel, dr), T(n_ent, d), T(n_rel, dr)], d, dr
    if kind == 'transh':
        return [T(n_ent, d), T(n_rel, d), T(n_rel, d)], d, d
    if kind == 'complex':
        return [T(n_ent, d), T(n_ent, d), T(n_rel, d), T(n_rel, d)], d, d
    if kind == 'rescal':
        return [T(n_ent, d), T(n_rel, d * d, 0.3)], d, d * d
    if kind == 'transr':
        dr = max(1, d - 3)
        return [T(n_ent, d), T(n_rel, dr), T(n_rel, dr * d, 0.3)], d, dr
    if kind in TORUS_DISS:
        return [rnd(g, n_ent, d) * 1.7, rnd(g, n_rel, d) * 1.7], d, d        # beyond (-1, 1): frac() has work to do
    return [T(n_ent, d), T(n_rel, d)], d, d


def triple_sf64(kind, T, de, dr, h, t, r):
    """float64 restatement of Model.scoring_function (differentiable in the tables)."""
    if kind in ('transe_l1', 'transe_l2'):
        return orc.score_triples('transe', T, h, t, r, p=1 if kind == 'transe_l1' else 2)
    if kind in ('transh', 'transd', 'distmult', 'complex'):
        return orc.score_triples(kind, T, h, t, r)
    if kind in ('rescal', 'hole'):
        return bilinear_sf64(kind, T[0], T[1], de, h, t, r)
    if kind == 'transr':
        return transr_sf64(T[0], T[1], T[2].view(-1, dr, de), h, t, r)

    def fr(x):
        return x - x.detach().trunc()
    return -diss64(TORUS_DISS[kind], (fr(T[0][h]) + fr(T[1][r])) - fr(T[0][t]))


def grad_close(got, want):
    err = (got.double().cpu() - want).abs().max().item()
    return err <= GRAD_TOL * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('d', [8, 17])
@pytest.mark.parametrize('kind', TRIPLE_KINDS)
def test_score_triples_and_backward_at_table_base_offsets(hip, kind, d):
    """kge_score_triples / kge_score_triples_bwd (row mode and atomic mode) for every kind with the contiguous tables 0..3
    floats off a 16-byte boundary (all at once, one at a time), d % 4 == 0 and != 0, h / t / r at an int64 offset; the
    gradient rows reduced by kge_segment_sum_rows / kge_rescal_rel_grad / kge_transr_rel_grad with padded ld / out_ld /
    ldg into guarded gradient tables: rows never indexed stay bit-zero, nothing outside a table is written."""
    lib = hip.load_library()
    code = TRIPLE_KINDS.index(kind)
    g = torch.Generator().manual_seed(code * 100 + d)
    tabs, de, dr = triple_tables(kind, d, g)
    n_ent, n_rel, nt, B = tabs[0].shape[0], tabs[2 if kind == 'complex' else 1].shape[0], len(tabs), 50
    h, t = torch.randint(0, n_ent - 5, (B,), generator=g), torch.randint(0, n_ent - 5, (B,), generator=g)
    r = torch.randint(0, n_rel - 1, (B,), generator=g)          # the last 5 entities / last relation are never indexed
    go = torch.randn(B, generator=g)
    T64 = [x.double().requires_grad_(True) for x in tabs]
    s64 = triple_sf64(kind, T64, de, dr, h, t, r)
    (s64 * go.double()).sum().backward()
    g64 = [x.grad for x in T64]
    ent_tables = {'complex': (0, 1), 'transd': (0, 2)}.get(kind, (0,))
    streams = hip._BWD_STREAMS.get(code, [(0, 0, 2, 'ht'), (1, 2, 1, 'r')])      # (TransR: rel_emb rides stream 2)
    W = max(de, dr) if kind == 'transr' else de
    base = None
    for offs in [[o] * nt for o in range(4)] + [[1 if i == j else 0 for i in range(nt)] for j in range(nt)]:
        tag = '%s d %d offsets %s' % (kind, d, offs)
        dt = [carve(x, 0, o, device='cuda') for x, o in zip(tabs, offs)] + [None] * (4 - nt)
        io = 0 if base is None else 1
        d_h, d_t = carve(h, off=io, poison=n_ent, device='cuda'), carve(t, off=io, poison=n_ent, device='cuda')
        d_r, d_go = carve(r, off=io, poison=n_rel, device='cuda'), carve(go, off=offs[0], device='cuda')
        out = guarded_out(B, off=offs[-1])
        assert raw(lib, 'kge_score_triples', code, dt[0], dt[1], dt[2], dt[3], de, dr, d_h, d_t, d_r, B, out) == 0, tag
        pad = 3
        rows = guarded_out(N_STREAMS.get(kind, 3) * B, W, pad, offs[0])
        ld = rows.stride(0)
        assert raw(lib, 'kge_score_triples_bwd', code, dt[0], dt[1], dt[2], dt[3], de, dr, d_h, d_t, d_r, B, d_go, None, None,
                   None, None, rows, ld) == 0, tag
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and close(out.cpu().numpy(), s64.detach().numpy()), tag
        got = {'out': out, 'rows': rows}
        grads = {}
        for ti, s0, ns, key in streams:
            gt = guarded_out(tabs[ti].shape[0], tabs[ti].shape[1], 2, offs[ti])
            gt.zero_()
            k0, n0, k1, n1 = (d_h, B, d_t, B) if key == 'ht' else (d_r, B, None, 0)
            perm = hip._key_perm(k0, k1, gt.shape[0])
            assert raw(lib, 'kge_segment_sum_rows', rows[s0 * B:], ld, gt.shape[1], k0, n0, k1, n1, perm, gt, gt.stride(0)) == 0, tag
            grads[ti] = gt
        if kind in ('rescal', 'transr'):
            ti = 1 if kind == 'rescal' else 2
            gM = guarded_out(n_rel, tabs[ti].shape[1], 1, offs[ti])
            perm = hip._key_perm(d_r, None, n_rel)
            if kind == 'rescal':
                rc = raw(lib, 'kge_rescal_rel_grad', rows[2 * B:], rows[3 * B:], ld, de, d_r, perm, B, n_rel, gM, gM.stride(0))
            else:
                rc = raw(lib, 'kge_transr_rel_grad', rows[2 * B:], ld, rows[3 * B:], ld, dr, de, d_r, perm, B, n_rel, gM,
                         gM.stride(0))
            assert rc == 0, tag
            grads[ti] = got['gM'] = gM
        torch.cuda.synchronize()
        for ti, gt in grads.items():
            assert bool(torch.isfinite(gt).all()) and grad_close(gt, g64[ti]), (tag, 'table', ti)
            never = slice(n_ent - 5, None) if ti in ent_tables else slice(n_rel - 1, None)
            assert not bits(gt[never]).any(), (tag, 'never-indexed rows of table', ti)
            assert_guard_intact(gt)
        if code < 6 or kind == 'hole':      # the atomic mode: added straight into caller-zeroed tables of the tables' shapes
            ga = [guarded_out(x.shape[0], x.shape[1], 0, o) for x, o in zip(tabs, offs)]
            for x in ga:
                x.zero_()
            ga4 = ga + [None] * (4 - nt)
            assert raw(lib, 'kge_score_triples_bwd', code, dt[0], dt[1], dt[2], dt[3], de, dr, d_h, d_t, d_r, B, d_go, ga4[0], ga4[1],
                       ga4[2], ga4[3], None, 0) == 0, tag
            torch.cuda.synchronize()
            for ti, gt in enumerate(ga):
                assert bool(torch.isfinite(gt).all()) and grad_close(gt, g64[ti]), (tag, 'atomic, table', ti)
                never = slice(n_ent - 5, None) if ti in ent_tables else slice(n_rel - 1, None)
                assert not bits(gt[never]).any(), (tag, 'atomic, never-indexed rows of table', ti)
                assert_guard_intact(gt)
        for v in [out, rows, d_h, d_t, d_r, d_go] + dt[:nt]:
            assert_guard_intact(v)
        base = True


def prep64(kind, T, dr, h, t, r):
    """float64 (Q0, Q1, Wq) of kge_lp_prep, side KGE_SIDE_BOTH (tail-side queries first), on the RAW tables."""
    T = [x.double() for x in T]
    if kind == 'transe_l2':
        E, R = T
        return torch.cat([E[h] + R[r], E[t] - R[r]]), None, None
    if kind == 'distmult':
        E, R = T
        return torch.cat([E[h] * R[r], R[r] * E[t]]), None, None
    if kind == 'complex':
        Er, Ei, Rr, Ri = T
        q0 = torch.cat([Er[h] * Rr[r] - Ei[h] * Ri[r], Rr[r] * Er[t] + Ri[r] * Ei[t]])
        q1 = torch.cat([Er[h] * Ri[r] + Ei[h] * Rr[r], Rr[r] * Ei[t] - Ri[r] * Er[t]])
        return q0, q1, None
    if kind == 'transh':
        E, R, Wn = T
        w = Wn[r]

        def p(e):
            return E[e] - (E[e] * w).sum(1, keepdim=True) * w
        return torch.cat([p(h) + R[r], p(t) - R[r]]), None, torch.cat([w, w])
    E, R, Ep, Rp = T
    w = Rp[r]

    def p(e):
        return (Ep[e] * E[e]).sum(1, keepdim=True) * w + E[e][:, :dr]
    return torch.cat([p(h) + R[r], p(t) - R[r]]), None, torch.cat([w, w])


@pytest.mark.parametrize('d', [8, 17])
@pytest.mark.parametrize('kind', ['transe_l2', 'transh', 'transd', 'distmult', 'complex'])
def test_lp_prep_family_at_table_base_offsets(hip, kind, d):
    """kge_lp_prep, kge_lp_prep_sharded (a real row shard: rows of entities it does not own come back as zeros) and
    kge_lp_prep_hi (TransH / TransD: the planar hi operand of the query rows rides along, the bytes kge_lp_hi_rows builds)
    with the contiguous tables 0..3 floats off a 16-byte boundary."""
    lib = hip.load_library()
    code = TRIPLE_KINDS.index(kind)
    g = torch.Generator().manual_seed(code * 10 + d)
    tabs, de, dr = triple_tables(kind, d, g)
    n_ent, n_rel, nt, B = tabs[0].shape[0], tabs[2 if kind == 'complex' else 1].shape[0], len(tabs), 45
    h, t, r = [torch.randint(0, n, (B,), generator=g) for n in (n_ent, n_ent, n_rel)]
    q0, q1, wq = prep64(kind, tabs, dr, h, t, r)
    lo, cnt = 7, 20
    ent_tables = {'complex': (0, 1), 'transd': (0, 2)}.get(kind, (0,))
    owned = torch.cat([(h >= lo) & (h < lo + cnt), (t >= lo) & (t < lo + cnt)]).view(-1, 1).double()
    proj = kind in ('transh', 'transd')
    base = None
    for offs in [[o] * nt for o in range(4)] + [[1 if i == j else 0 for i in range(nt)] for j in range(nt)]:
        tag = '%s d %d offsets %s' % (kind, d, offs)
        dt = [carve(x, 0, o, device='cuda') for x, o in zip(tabs, offs)] + [None] * (4 - nt)
        ds = [carve(x[lo:lo + cnt] if i in ent_tables else x, 0, o, device='cuda') for i, (x, o) in enumerate(zip(tabs, offs))]
        ds += [None] * (4 - nt)
        d_h, d_t = carve(h, off=1, poison=n_ent, device='cuda'), carve(t, off=1, poison=n_ent, device='cuda')
        d_r = carve(r, off=1, poison=n_rel, device='cuda')

        def outs():
            return (guarded_out(2 * B, dr), guarded_out(2 * B, dr) if kind == 'complex' else None, guarded_out(2 * B, off=offs[0]),
                    guarded_out(2 * B, dr) if proj else None)
        Q0, Q1, qn, Wq = outs()
        assert raw(lib, 'kge_lp_prep', code, hip.SIDE_BOTH, dt[0], dt[1], dt[2], dt[3], de, dr, d_h, d_t, d_r, B, Q0, Q1, qn, Wq) == 0, tag
        S0, S1, _, Sw = outs()
        assert raw(lib, 'kge_lp_prep_sharded', code, hip.SIDE_BOTH, ds[0], ds[1], ds[2], ds[3], de, dr, d_h, d_t, d_r, B, lo, cnt,
                   S0, S1, None, Sw) == 0, tag
        got = {'Q0': Q0, 'qn': qn, 'S0': S0}
        if kind == 'complex':
            got['Q1'], got['S1'] = Q1, S1
        if proj:
            got['Wq'], got['Sw'] = Wq, Sw
            units_p, Bp = int(lib.kge_lp_hi_units(dr)), int(lib.kge_lp_split_rows_padded(2 * B, 1))
            H0, _, hn, Hw = outs()
            Qh, dn2 = guarded_out(Bp * units_p * 32, dtype=torch.uint8), guarded_out(2 * B, off=1)
            assert raw(lib, 'kge_lp_prep_hi', code, hip.SIDE_BOTH, dt[0], dt[1], dt[2], dt[3], de, dr, d_h, d_t, d_r, B, 0, -1, H0,
                       None, hn, Hw, Qh, units_p, Bp, dn2) == 0, tag
            Qh_ref, dn2_ref = guarded_out(Bp * units_p * 32, dtype=torch.uint8), guarded_out(2 * B, off=3)
            assert raw(lib, 'kge_lp_hi_rows', Q0, dr, dr, None, 0, 0, 2 * B, 1, 2, None, ctypes.c_float(1.0), None, None, Qh_ref,
                       dn2_ref, None, None) == 0, tag
            torch.cuda.synchronize()
            assert same_bits(H0, Q0) and same_bits(hn, qn) and same_bits(Hw, Wq), tag
            live = 2 * B * units_p * 32      # (the bytes of the 2B query rows)
            assert torch.equal(Qh[:live], Qh_ref[:live]) and _near(dn2, dn2_ref), tag
            got['Qh'] = Qh
            for v in (H0, hn, Hw, Qh, dn2, Qh_ref, dn2_ref):
                assert_guard_intact(v)
        torch.cuda.synchronize()
        for v in got.values():
            assert bool(torch.isfinite(v.float()).all()), tag
            assert_guard_intact(v)
        assert close(Q0.cpu().numpy(), q0.numpy()) and close(qn.cpu().numpy(), (q0 * q0).sum(1).numpy()), tag
        assert close(S0.cpu().numpy(), (q0 * owned).numpy()), tag
        if kind == 'complex':
            assert close(Q1.cpu().numpy(), q1.numpy()) and close(S1.cpu().numpy(), (q1 * owned).numpy()), tag
        if proj:
            assert close(Wq.cpu().numpy(), wq.numpy()) and close(Sw.cpu().numpy(), wq.numpy()), tag
        for v in [d_h, d_t, d_r] + dt[:nt] + ds[:nt]:
            assert_guard_intact(v)
        base = True


# ---------------------------------------------------------------------------
# F. query transforms
# ---------------------------------------------------------------------------
def _pad_combos(n):
    """(pad, off) per operand: every operand at once (FEW + two odd ones), then one operand at a time."""
    out = [[po] * n for po in FEW + [(1, 0), (0, 1)]]
    for j in range(n):
        for po in ((1, 0), (0, 3), (4, 0)):
            out.append([po if i == j else (0, 0) for i in range(n)])
    return out


@pytest.mark.parametrize('de,dr', [(1, 1), (8, 5), (17, 32), (32, 24), (64, 64)])
def test_transr_transforms_with_padded_leading_dimensions(hip, de, dr):
    """kge_transr_proj_sqnorm (ldm, ldx, ldb; both output orientations through os_r / os_j) and kge_transr_query (ldx, ldm,
    ldr, ldq, ldu) with every leading dimension padded and every base offset."""
    from tests.test_gpu_transr import random_tables
    lib = hip.load_library()
    n_ent, n_rel, B = 70, 5, 90
    E, R, P = random_tables(n_ent, n_rel, de, dr, seed=de * 1000 + dr)
    g = torch.Generator().manual_seed(de + dr)
    h, t, r = [torch.randint(0, n, (B,), generator=g) for n in (n_ent, n_ent, n_rel)]
    M64 = P.double().view(n_rel, dr, de)
    p = torch.einsum('rck,nk->rnc', M64, E.double()) + R.double().unsqueeze(1)
    z64 = (p * p).sum(2)
    qt = torch.einsum('bck,bk->bc', M64[r], E.double()[h]) + R.double()[r]
    qh = torch.einsum('bck,bk->bc', M64[r], E.double()[t]) - R.double()[r]
    q64 = torch.cat([qt, qh])
    u64 = torch.einsum('bck,bc->bk', torch.cat([M64[r], M64[r]]), q64)
    base = None
    for (pm, om), (px, ox), (pb, ob) in _pad_combos(3):
        tag = 'M %d.%d X %d.%d R %d.%d' % (pm, om, px, ox, pb, ob)
        dP, dE, dR = carve(P, pm, om, device='cuda'), carve(E, px, ox, device='cuda'), carve(R, pb, ob, device='cuda')
        d_h, d_t = carve(h, off=1, poison=n_ent, device='cuda'), carve(t, off=1, poison=n_ent, device='cuda')
        d_r = carve(r, off=1, poison=n_rel, device='cuda')
        Z, Zt = guarded_out(n_rel, n_ent, pm + 1, ox), guarded_out(n_ent, n_rel, px, om)
        args = (dP, dP.stride(0), dE, dE.stride(0), dR, dR.stride(0), None, n_rel, n_ent, de, dr)
        assert raw(lib, 'kge_transr_proj_sqnorm', *(args + (Z, Z.stride(0), 1))) == 0, tag
        assert raw(lib, 'kge_transr_proj_sqnorm', *(args + (Zt, 1, Zt.stride(0)))) == 0, tag
        perm = hip._key_perm(d_r, d_r, n_rel)
        Q, U = guarded_out(2 * B, dr, pb, ob), guarded_out(2 * B, de, px + 1, ox)
        assert raw(lib, 'kge_transr_query', hip.SIDE_BOTH, dE, dE.stride(0), dP, dP.stride(0), dR, dR.stride(0), de, dr, d_h, d_t,
                   d_r, B, perm, Q, Q.stride(0), U, U.stride(0)) == 0, tag
        torch.cuda.synchronize()
        got = {'Z': Z, 'Zt': Zt, 'Q': Q, 'U': U}
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), (tag, k)
            assert_guard_intact(v)
        assert close(Z.cpu().numpy(), z64.numpy()) and close(Zt.cpu().numpy(), z64.t().numpy()), tag
        assert close(Q.cpu().numpy(), q64.numpy()) and close(U.cpu().numpy(), u64.numpy()), tag
        for v in (dP, dE, dR, d_h, d_t, d_r):
            assert_guard_intact(v)
        if base is None:
            base = {k: v.clone() for k, v in got.items()}
        for k, v in got.items():        # the header's order contract: a value depends on (relation, row) only
            assert same_bits(v, base[k]), (tag, k)


@pytest.mark.parametrize('d', [1, 8, 17, 64])
@pytest.mark.parametrize('kind', ['rescal', 'hole'])
def test_bilinear_transforms_with_padded_leading_dimensions(hip, kind, d):
    """kge_bilinear_query (ldx, ldr, ldq) and kge_bilinear_relation_rows (ldh, ldt, ldo) with every leading dimension
    padded and every base offset; RESCAL's relation rows are single products and compared bit for bit."""
    lib = hip.load_library()
    code = hip.RESCAL if kind == 'rescal' else hip.HOLE
    n_ent, n_rel, B = 60, 5, 80
    g = torch.Generator().manual_seed(d * 3 + code)
    E = torch.randn(n_ent, d, generator=g) * 0.5
    rel = torch.randn(n_rel, d * d if kind == 'rescal' else d, generator=g) * 0.3
    h, t, r = [torch.randint(0, n, (B,), generator=g) for n in (n_ent, n_ent, n_rel)]
    q64 = torch.cat([queries64(kind, E, rel, d, h, r, 'tail'), queries64(kind, E, rel, d, t, r, 'head')])
    H, T = E[h].contiguous(), E[t].contiguous()
    if kind == 'rescal':
        rows_ref = (H.unsqueeze(2) * T.unsqueeze(1)).reshape(B, d * d)
    else:
        jk = (torch.arange(d).view(d, 1) + torch.arange(d).view(1, d)) % d
        rows_ref = torch.einsum('bj,bjk->bk', H.double(), T.double()[:, jk])
    wo = rows_ref.shape[1]
    base = None
    for (px, ox), (pr, orr), (ph, oh) in _pad_combos(3):
        tag = 'X %d.%d rel %d.%d H/T %d.%d' % (px, ox, pr, orr, ph, oh)
        dE, dRel = carve(E, px, ox, device='cuda'), carve(rel, pr, orr, device='cuda')
        d_h, d_t = carve(h, off=1, poison=n_ent, device='cuda'), carve(t, off=1, poison=n_ent, device='cuda')
        d_r = carve(r, off=1, poison=n_rel, device='cuda')
        perm = hip._key_perm(d_r, d_r, n_rel)
        Q = guarded_out(2 * B, d, pr + 1, orr)
        assert raw(lib, 'kge_bilinear_query', code, hip.SIDE_BOTH, dE, dE.stride(0), dRel, dRel.stride(0), d, d_h, d_t, d_r, B, 0, -1,
                   perm, Q, Q.stride(0)) == 0, tag
        dH, dT = carve(H, ph, oh, device='cuda'), carve(T, px, ox, device='cuda')
        out = guarded_out(B, wo, pr, oh)
        assert raw(lib, 'kge_bilinear_relation_rows', code, dH, dH.stride(0), dT, dT.stride(0), B, d, out, out.stride(0)) == 0, tag
        torch.cuda.synchronize()
        got = {'Q': Q, 'rows': out}
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), (tag, k)
            assert_guard_intact(v)
        assert close(Q.cpu().numpy(), q64.numpy()), tag
        if kind == 'rescal':
            assert same_bits(out.cpu(), rows_ref), tag
        else:
            assert close(out.cpu().numpy(), rows_ref.numpy()), tag
        for v in (dE, dRel, dH, dT, d_h, d_t, d_r):
            assert_guard_intact(v)
        if base is None:
            base = Q.clone()
        assert same_bits(Q, base), tag      # one ascending chain per output: a row depends on (entity, relation, side) only


@pytest.mark.parametrize('kind,de,dr', [('transh', 8, 8), ('transh', 17, 17), ('transd', 12, 8), ('transd', 17, 6), ('transd', 64, 64)])
def test_relation_scores_proj_at_base_offsets_into_a_padded_output(hip, kind, de, dr):
    """kge_relation_scores_proj: contiguous tables 0..3 floats off a 16-byte boundary, the (B, n_rel) output with ldo > n_rel."""
    lib = hip.load_library()
    code = hip.TRANSH if kind == 'transh' else hip.TRANSD
    n_ent, n_rel, B = 50, 7, 60
    g = torch.Generator().manual_seed(de * 7 + dr)
    E, R, Wt = [torch.randn(n, k, generator=g) * 0.4 for n, k in ((n_ent, de), (n_rel, dr), (n_rel, dr))]
    Ep = torch.randn(n_ent, de, generator=g) * 0.4 if kind == 'transd' else None
    h, t = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, n_ent, (B,), generator=g)
    E6, R6, W6 = E.double(), R.double(), Wt.double()

    def p(e):       # (B, n_rel, d_r): the projection of entity row e under every relation
        if kind == 'transh':
            return E6[e].unsqueeze(1) - (E6[e] @ W6.t()).unsqueeze(2) * W6.unsqueeze(0)
        s = (Ep.double()[e] * E6[e]).sum(1)
        return s.view(-1, 1, 1) * W6.unsqueeze(0) + E6[e][:, :dr].unsqueeze(1)
    ref = -((p(h) + R6.unsqueeze(0) - p(t)) ** 2).sum(2)
    tabs = [E, R, Wt] + ([Ep] if Ep is not None else [])
    nt = len(tabs)
    base = None
    for offs in [[o] * nt for o in range(4)] + [[1 if i == j else 0 for i in range(nt)] for j in range(nt)]:
        dt = [carve(x, 0, o, device='cuda') for x, o in zip(tabs, offs)] + [None] * (4 - nt)
        d_h, d_t = carve(h, off=1, poison=n_ent, device='cuda'), carve(t, off=1, poison=n_ent, device='cuda')
        out = guarded_out(B, n_rel, 1 + offs[0], offs[-1])
        assert raw(lib, 'kge_relation_scores_proj', code, dt[0], dt[1], dt[2], dt[3], de, dr, d_h, d_t, B, n_rel, out,
                   out.stride(0)) == 0, offs
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and close(out.cpu().numpy(), ref.numpy()), offs
        for v in [out, d_h, d_t] + dt[:nt]:
            assert_guard_intact(v)


@pytest.mark.parametrize('K', [1, 8, 17, 64])
def test_lp_scores_batched_strides(hip, K):
    """kge_lp_scores_batched: ldq, stride_b (per-query candidate matrices, and 0: shared), stride_n and ldo all padded, bases
    offset; every mode it takes, against the float64 restatement (lanes over k: no chain contract)."""
    lib = hip.load_library()
    B, N = 7, 33
    g = torch.Generator().manual_seed(K)
    q, cand = rnd(g, B, K) * 0.5, rnd(g, B, N, K) * 0.5         # x = q - c in (-1, 1): non-negative torus terms
    x = (q.view(B, 1, K) - cand).double()
    x0 = (q.view(B, 1, K) - cand[0].view(1, N, K)).double()

    def ref(mode, xx, c):
        if mode == hip.LP_DOT:
            return torch.einsum('bk,bnk->bn', q.double(), c.double().expand(B, N, K))
        if mode == hip.LP_L1_DIRECT:
            return -xx.abs().sum(-1)
        if mode == hip.LP_L2_DIRECT:
            return -(xx ** 2).sum(-1)
        if mode == hip.LP_TORUS_L1:
            return -2 * torch.minimum(xx.abs(), 1 - xx.abs()).sum(-1)
        if mode == hip.LP_TORUS_L2:
            return -4 * torch.minimum(xx ** 2, 1 - xx ** 2).sum(-1)
        return -(2 * (1 - torch.cos(2 * math.pi * torch.minimum(xx, 1 - xx)))).sum(-1) / 4
    base = {}
    for (pq, oq), (pc, oc), (po, oo) in _pad_combos(3):
        dq = carve(q, pq, oq, device='cuda')
        dc = carve(cand.reshape(B * N, K), pc, oc, device='cuda')
        dc0 = carve(cand[0], pc, oc, device='cuda')
        for mode in (hip.LP_DOT, hip.LP_L1_DIRECT, hip.LP_L2_DIRECT, hip.LP_TORUS_L1, hip.LP_TORUS_L2, hip.LP_TORUS_EL2):
            for shared in (False, True):
                tag = (mode, shared, pq, oq, pc, oc, po, oo)
                c, sn = (dc0, dc0.stride(0)) if shared else (dc, dc.stride(0))
                out = guarded_out(B, N, po, oo)
                assert raw(lib, 'kge_lp_scores_batched', mode, dq, dq.stride(0), c, 0 if shared else N * sn, sn, B, N, K, out,
                           out.stride(0)) == 0, tag
                torch.cuda.synchronize()
                want = ref(mode, x0 if shared else x, cand[0:1] if shared else cand)
                assert bool(torch.isfinite(out).all()) and close(out.cpu().numpy(), want.numpy()), tag
                assert_guard_intact(out)
        for v in (dq, dc, dc0):
            assert_guard_intact(v)


def test_region_recheck_on_a_padded_descriptor_and_its_refusal(hip):
    """kge_lp_split_recheck_regions re-scores the listed pairs with the exact-score descriptor: with Q / E carved at padded,
    16-byte aligned leading dimensions the counts are the exact ones; a descriptor whose rows are not float4-readable
    (kge_lp_split_regions_supported: 0) is refused with KGE_EINVAL before anything is launched."""
    lib = hip.load_library()
    B, N, d = 70, 600, 64
    g = torch.Generator().manual_seed(17)
    E = torch.nn.functional.normalize(torch.randn(N, d, generator=g), dim=1).cuda()
    R = (0.3 * torch.randn(5, d, generator=g)).cuda()
    h, t, r = [torch.randint(0, n, (B,), generator=g).cuda() for n in (N, N, 5)]
    true = torch.cat([t, h])
    want = None
    for pq, pe in ((0, 0), (4, 8), (8, 4)):
        guard = torch.zeros(8, device='cuda')
        en, Ef, tpb = hip.table_prep_l2(E, guard[1:2], guard[7:8], deferred_max=True)
        pre = hip.lp_query_pipeline(hip.SIDE_BOTH, E, R, h, t, r, en, guard[1:2], guard[0:1], level=1, de2max=guard[7:8],
                                    tp_bmax=tpb, zero_counts=True, regions=True)
        assert pre.get('region_count') is not None
        pre['true_idx'] = true
        dQ, dE = carve(pre['Q'].cpu(), pq, 0, device='cuda'), carve(E.cpu(), pe, 0, device='cuda')
        prob = hip.LpProblem(hip.LP_L2_EXPAND, dQ, dE, qn=pre['qn'], en=en)
        assert int(lib.kge_lp_split_regions_supported(ctypes.byref(prob.desc))) == 1
        prob.split = {'Es': Ef, 'e2pref': None, 'enmax': guard[1:2], 'overflow': guard[2:3], 'level': 1, 'de2max': guard[7:8],
                      'list_stat': guard[6:7], 'es_frag': True}
        prob.pre = pre
        st = prob.pair_scores(true)
        got = prob.count_ge(st).clone()
        exact = hip.LpProblem(hip.LP_L2_EXPAND, dQ, dE, qn=pre['qn'], en=en).count_ge(st)
        torch.cuda.synchronize()
        assert float(guard[2]) == 0.0 and int(pre['region_count'].sum()) == int(prob.last_split[0]) > 0
        assert torch.equal(got, exact)
        if want is None:
            want = got
        assert torch.equal(got, want), (pq, pe)
        assert_guard_intact(dQ)
        assert_guard_intact(dE)
    n_reg = int(lib.kge_lp_split_regions(2 * B))
    for lay in ({'A0': (1, 0)}, {'T0': (3, 0)}, {'A0': (0, 1)}, {'T0': (0, 2)}):
        ops = {'A0': pre['Q'].cpu(), 'T0': E.cpu(), 'qn': pre['qn'].cpu(), 'en': en.cpu()}
        bad, dv = problem(hip, 'l2x', ops, lay)
        assert int(lib.kge_lp_split_regions_supported(ctypes.byref(bad.desc))) == 0, lay
        cnt = guarded_out(2 * B, dtype=torch.int32)
        lst, rc_ = torch.zeros(n_reg * 8 * 2, dtype=torch.int32, device='cuda'), torch.ones(n_reg, dtype=torch.int32, device='cuda')
        assert raw(lib, 'kge_lp_split_recheck_regions', bad.desc, st, lst, n_reg * 8, rc_, cnt, None, None) == KGE_EINVAL, lay
        torch.cuda.synchronize()
        assert_guard_intact(cnt, rows=0)
