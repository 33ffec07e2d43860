"""GPU tests of KGE_LP_CMOD (include/kge_hip_rotate.h) through the C ABI (run with -m gpu on an MI355X): kge_lp_scores
against float64 on the same fp32 operands, and bit-for-bit agreement of kge_lp_pair_scores, the scores inside
kge_lp_count_ge and kge_lp_filter_sub with the score matrix, at the smallest shapes where the 128 x 128 tile with
BK = 32 can go wrong, on packed, padded and unaligned operands; the refusals; kge_rotate_query and the triple kernel
against the mode."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import carve, guarded_out, assert_guard_intact, raw
from tests import rotate_ref as ref
from tests.test_gpu_toruse import TOL, close      # the direct family's score tolerance: |a - ref| < 1e-5 max(1, |ref|)

pytestmark = pytest.mark.gpu

NAN = float('nan')
EINVAL = -1     # KGE_EINVAL of include/kge_hip.h
C_BASE = 5
# K0: a lone pair; a last 4-group of one pair and one absent pair; exactly one slice; a non-multiple of 4 (the scalar
# fetch path); two slices on the 16-byte path; three slices
KS = (2, 6, 32, 34, 36, 72)
SHAPES = ((1, 1), (129, 129), (130, 257))
# (pad of A0, offset of A0 in floats, pad of T0, offset of T0): packed; padded leading dimensions that keep 16-byte rows;
# padded ones that do not; an unaligned base
LAYOUTS = ((0, 0, 0, 0), (4, 0, 8, 0), (1, 0, 3, 0), (0, 1, 0, 3), (4, 2, 0, 0))


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip, _hip_rotate
    _hip_rotate.load_library()
    return _hip


def operands(B, N, K, seed=0):
    g = torch.Generator().manual_seed(1000 * K + 10 * B + N + seed)
    A = torch.rand(B, K, generator=g) * 2 - 1
    T = torch.rand(N, K, generator=g) * 2 - 1
    return A, T


def problem(hip, A, T, lay=(0, 0, 0, 0), c_base=0):
    dA, dT = carve(A, lay[0], lay[1], NAN, device='cuda'), carve(T, lay[2], lay[3], NAN, device='cuda')
    prob = hip.LpProblem(hip.LP_CMOD, dA, dT, c_base=c_base)
    assert (prob.desc.lda0, prob.desc.ldt0) == (A.shape[1] + lay[0], T.shape[1] + lay[2])
    assert prob.desc.A0 % 16 == 4 * lay[1] and prob.desc.T0 % 16 == 4 * lay[3]
    return prob, (dA, dT)


def scores(hip, prob, pad=0, off=0):
    out = guarded_out(prob.B, prob.N, pad, off)
    assert raw(hip.load_library(), 'kge_lp_scores', prob.desc, out, out.stride(0)) == 0
    torch.cuda.synchronize()
    assert_guard_intact(out)
    return out


@pytest.fixture(scope='module')
def matrices(hip):
    """The packed score matrix of every (K, B, N), computed once and checked against float64; shared, never written."""
    out = {}
    for K in KS:
        for B, N in SHAPES:
            A, T = operands(B, N, K)
            prob, _ = problem(hip, A, T)
            S = scores(hip, prob).clone()
            assert bool(torch.isfinite(S).all())
            assert close(S.cpu(), ref.cmod_scores64(A, T)), (K, B, N)
            out[(K, B, N)] = (A, T, S)
    return out


@pytest.mark.parametrize('K', KS)
def test_scores_vs_float64_and_every_layout_gives_the_same_bits(hip, matrices, K):
    for B, N in SHAPES:
        A, T, S = matrices[(K, B, N)]
        for i, lay in enumerate(LAYOUTS[1:]):
            prob, dv = problem(hip, A, T, lay)
            got = scores(hip, prob, pad=(0, 1, 4, 5)[i], off=i)
            assert torch.equal(got.view(torch.int32), S.view(torch.int32)), (K, B, N, lay)
            for v in dv:
                assert_guard_intact(v)


def filter_fixture(g, B, N, true_loc):
    """One distinct non-empty segment of GLOBAL ids per query, some ids outside the shard, every other one holding the
    true entity."""
    lo, hi, tg = [], [], []
    for i in range(B):
        n = int(torch.randint(1, 7, (1,), generator=g))
        ids = torch.randint(0, N + 2 * C_BASE, (n,), generator=g).tolist()
        if i % 2 == 0:
            ids[0] = int(true_loc[i]) + C_BASE
        ids = sorted(set(ids))
        lo.append(len(tg))
        tg.extend(ids)
        hi.append(len(tg))
    return torch.tensor(lo), torch.tensor(hi), torch.tensor(tg, dtype=torch.int32)


def filter_expect(S, st, true_glob, lo, hi, tg, N):
    B = S.shape[0]
    sub, found = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for i in range(B):
        for gid in tg[int(lo[i]):int(hi[i])].tolist():
            c = gid - C_BASE
            if c < 0 or c >= N:
                continue
            if gid == int(true_glob[i]):
                found[i] = 1
            else:
                sub[i] += int(S[i, c] >= st[i])
    return sub, found


@pytest.mark.parametrize('K', KS)
def test_pair_count_and_filter_kernels_give_the_bits_of_the_score_matrix(hip, matrices, K):
    """All pairs through kge_lp_pair_scores; kge_lp_count_ge against thresholds taken from the matrix itself (a count that
    scored a pair differently would miss or gain the ties the threshold makes: the true entity at least); kge_lp_filter_sub
    from the same thresholds -- on packed operands (the staged float4 chain where K % 4 == 0) and on padded / unaligned ones
    (the scalar chain)."""
    lib = hip.load_library()
    for B, N in SHAPES:
        A, T, S = matrices[(K, B, N)]
        Sn = S.cpu().numpy()
        g = torch.Generator().manual_seed(K + B + N)
        true_loc = torch.randint(0, N, (B,), generator=g)
        st = Sn[np.arange(B), true_loc.numpy()].copy()
        cnt_ref = (Sn >= st[:, None]).sum(1).astype(np.int32)
        lo, hi, tg = filter_fixture(g, B, N, true_loc)
        sub_ref, found_ref = filter_expect(Sn, st, true_loc + C_BASE, lo, hi, tg, N)
        qi = torch.arange(B).repeat_interleave(N)
        ci = torch.arange(N).repeat(B) + C_BASE
        for lay in (LAYOUTS[0], LAYOUTS[2], LAYOUTS[3]):
            prob, dv = problem(hip, A, T, lay, c_base=C_BASE)
            d_qi, d_ci = qi.cuda(), ci.cuda()
            po = guarded_out(B * N)
            assert raw(lib, 'kge_lp_pair_scores', prob.desc, d_qi, d_ci, B * N, po) == 0
            d_st = torch.from_numpy(st).cuda()
            cnt = torch.zeros(B, dtype=torch.int32, device='cuda')
            assert raw(lib, 'kge_lp_count_ge', prob.desc, d_st, cnt) == 0
            sub, found = guarded_out(B, dtype=torch.int32), guarded_out(B, dtype=torch.int32)
            assert raw(lib, 'kge_lp_filter_sub', prob.desc, d_st, (true_loc + C_BASE).cuda(), lo.cuda(), hi.cuda(), tg.cuda(),
                       sub, found) == 0
            torch.cuda.synchronize()
            tag = (K, B, N, lay)
            assert torch.equal(po.view(B, N).view(torch.int32), S.view(torch.int32)), tag
            assert np.array_equal(cnt.cpu().numpy(), cnt_ref), tag
            assert np.array_equal(sub.cpu().numpy(), sub_ref) and np.array_equal(found.cpu().numpy(), found_ref), tag
            for v in (po, sub, found) + dv:
                assert_guard_intact(v)


@pytest.mark.parametrize('K', KS)
def test_equal_rows_score_zero_and_nothing_is_nan(hip, K):
    """q == e in every coordinate: every modulus is sqrt(0) = 0 and the score is exactly +-0; a pair that differs in ONE
    component (the other of its complex coordinate equal) scores that difference exactly."""
    A, T = operands(130, 257, K, seed=7)
    T[3] = A[0]
    T[200] = A[129]
    T[5] = A[1]
    T[5, K - 1] += 0.5
    prob, _ = problem(hip, A, T)
    S = scores(hip, prob).cpu()
    assert not bool(torch.isnan(S).any())
    assert float(S[0, 3]) == 0.0 and float(S[129, 200]) == 0.0
    assert float(S[1, 5]) == -float(abs(A[1, K - 1] - T[5, K - 1]))
    pairs = hip.LpProblem(hip.LP_CMOD, A.cuda(), T.cuda()).pair_scores(torch.tensor([3, 200, 5]).cuda(),
                                                                      torch.tensor([0, 129, 1]).cuda()).cpu()
    assert torch.equal(pairs.view(torch.int32), torch.stack([S[0, 3], S[129, 200], S[1, 5]]).view(torch.int32))


def test_refusals(hip):
    lib = hip.load_library()
    A, T = operands(4, 6, 8)
    out = guarded_out(4, 6)
    for K0 in (7, 5, 1):            # an odd K0
        prob, _ = problem(hip, A, T)
        prob.desc.K0 = K0
        assert raw(lib, 'kge_lp_scores', prob.desc, out, out.stride(0)) == EINVAL
        cnt = torch.zeros(4, dtype=torch.int32, device='cuda')
        assert raw(lib, 'kge_lp_count_ge', prob.desc, torch.zeros(4, device='cuda'), cnt) == EINVAL
        assert raw(lib, 'kge_lp_pair_scores', prob.desc, None, torch.zeros(4, dtype=torch.int64, device='cuda'), 4,
                   torch.zeros(4, device='cuda')) == EINVAL
    prob = hip.LpProblem(hip.LP_CMOD, A.cuda(), T.cuda(), A1=A.cuda(), T1=T.cuda())     # K1 > 0
    assert prob.desc.K1 == 8
    assert raw(lib, 'kge_lp_scores', prob.desc, out, out.stride(0)) == EINVAL
    prob = hip.LpProblem(hip.LP_CMOD, A.cuda(), T.cuda(), Wq=A.cuda(), scal=torch.zeros(6, device='cuda'))   # a rank-1 term
    assert raw(lib, 'kge_lp_scores', prob.desc, out, out.stride(0)) == EINVAL
    # the batched kernel: an odd K is refused, an even one gives the mode's values
    q, c = A.cuda(), T.cuda().view(1, 6, 8).expand(4, 6, 8).contiguous()
    assert raw(lib, 'kge_lp_scores_batched', hip.LP_CMOD, q, 8, c, 48, 8, 4, 6, 7, out, out.stride(0)) == EINVAL
    torch.cuda.synchronize()
    assert_guard_intact(out, rows=0)
    assert close(hip.lp_scores_batched(hip.LP_CMOD, q, c).cpu(), ref.cmod_scores64(A, T))


@pytest.mark.parametrize('d', [1, 3, 16, 17, 100])
def test_query_rows_and_triple_scores_have_the_bits_of_the_mode(hip, d):
    """kge_rotate_query against float64 (both sides, padded tables, a row shard); the head-side rows score what the
    definition |c r - t| gives; kge_score_triples has the bits of the KGE_LP_CMOD pair score of the tail-side row against
    the tail."""
    from torchkge_amd import _hip_rotate
    lib = _hip_rotate.load_library()
    g = torch.Generator().manual_seed(d)
    n_ent, n_rel, B = 61, 4, 150
    E = torch.rand(n_ent, 2 * d, generator=g) * 2 - 1
    P = (torch.rand(n_rel, d, generator=g) * 2 - 1) * math.pi
    h, t, r = (torch.randint(0, n, (B,), generator=g) for n in (n_ent, n_ent, n_rel))
    Ed, Pd, hd, td, rd = E.cuda(), P.cuda(), h.cuda(), t.cuda(), r.cuda()
    Q = _hip_rotate.rotate_query(hip.SIDE_BOTH, Ed, Pd, hd, td, rd)
    assert tuple(Q.shape) == (2 * B, 2 * d)
    want = torch.cat([torch.view_as_real(ref.queries64(E, P, h, t, r, s)).reshape(B, 2 * d) for s in ('tail', 'head')])
    assert float((Q.cpu().double() - want).abs().max()) < 4e-7      # two roundings of products of |x| <= 1 beside sincosf's
    assert torch.equal(Q[:B], _hip_rotate.rotate_query(hip.SIDE_TAIL, Ed, Pd, hd, td, rd))
    assert torch.equal(Q[B:], _hip_rotate.rotate_query(hip.SIDE_HEAD, Ed, Pd, hd, td, rd))
    # padded leading dimensions and unaligned bases: the same bits, nothing outside the rows written
    cE, cP = carve(E, 3, 1, NAN, device='cuda'), carve(P, 1, 3, NAN, device='cuda')
    out = guarded_out(2 * B, 2 * d, 5, 1)
    assert raw(lib, 'kge_rotate_query', hip.SIDE_BOTH, cE, cE.stride(0), cP, cP.stride(0), d, hd, td, rd, B, 0, -1, out,
               out.stride(0)) == 0
    torch.cuda.synchronize()
    assert_guard_intact(out)
    assert torch.equal(out.view(torch.int32), Q.view(torch.int32))
    # a row shard: rows of entities outside [20, 45) come back as zeros, the others with the same bits
    lo, n = 20, 25
    Qs = _hip_rotate.rotate_query(hip.SIDE_BOTH, Ed[lo:lo + n], Pd, hd, td, rd, ent_lo=lo, ent_n=n)
    own = torch.cat([(h >= lo) & (h < lo + n), (t >= lo) & (t < lo + n)]).cuda()
    assert torch.equal(Qs[own], Q[own]) and not bool(Qs[~own].any()) and bool(own.any()) and bool((~own).any())
    # refusals
    for args in ((9, Ed, 2 * d, Pd, d, d), (hip.SIDE_TAIL, Ed, 2 * d - 1, Pd, d, d), (hip.SIDE_TAIL, Ed, 2 * d, Pd, d - 1, d),
                 (hip.SIDE_TAIL, Ed, 2 * d, Pd, d, 0)):
        assert raw(lib, 'kge_rotate_query', args[0], args[1], args[2], args[3], args[4], args[5], hd, td, rd, B, 0, -1, Q,
                   Q.stride(0)) == EINVAL
    # scores of the rows
    prob = hip.LpProblem(hip.LP_CMOD, Q, Ed)
    S = prob.scores().cpu()
    assert close(S[:B], ref.scores64(E, P, h, t, r, 'tail')) and close(S[B:], ref.scores64(E, P, h, t, r, 'head'))
    sf = hip.score_triples(hip.ROTATE, [Ed, Pd], 2 * d, d, hd, td, rd)
    assert close(sf.cpu(), ref.sf64(E, P, h, t, r))
    assert torch.equal(sf.view(torch.int32), prob.pair_scores(td, torch.arange(B).cuda()).view(torch.int32))
    assert torch.equal(sf.cpu().view(torch.int32), S[torch.arange(B), t].view(torch.int32))


def test_triple_kind_refusals(hip):
    lib = hip.load_library()
    E, P = torch.zeros(5, 8, device='cuda'), torch.zeros(2, 4, device='cuda')
    i = torch.zeros(3, dtype=torch.int64, device='cuda')
    out = torch.zeros(3, device='cuda')
    ok = lambda de, dr: raw(lib, 'kge_score_triples', hip.ROTATE, E, P, None, None, de, dr, i, i, i, 3, out)   # noqa: E731
    assert ok(8, 4) == 0 and ok(8, 8) == EINVAL and ok(4, 4) == EINVAL and ok(1026, 513) == EINVAL
    # the backward has the row mode only
    g = torch.zeros(5, 8, device='cuda')
    assert raw(lib, 'kge_score_triples_bwd', hip.ROTATE, E, P, None, None, 8, 4, i, i, i, 3, out, g, torch.zeros(2, 4, device='cuda'),
               None, None, None, 0) == EINVAL
    rows = torch.zeros(9 * 8, device='cuda')
    assert raw(lib, 'kge_score_triples_bwd', hip.ROTATE, E, P, None, None, 8, 4, i, i, i, 3, out, None, None, None, None,
               rows, 7) == EINVAL
    assert raw(lib, 'kge_score_triples_bwd', hip.ROTATE, E, P, None, None, 8, 4, i, i, i, 3, out, None, None, None, None,
               rows, 8) == 0
    torch.cuda.synchronize()
