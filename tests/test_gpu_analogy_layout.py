"""The LAYOUT contract of include/kge_hip_analogy.h on the MI355X, in the manner of tests/test_gpu_layout_contract.py:
every input table is a view carved out of one poisoned buffer (row stride d + pad, pad in {0, 1, 3, 4, 8}; base 0..3
floats past a 16-byte boundary) -- all operands at once, and one operand at a time with the rest packed and aligned --
index vectors sit one element off, outputs lie in sentinel-filled buffers with a padded leading dimension.  Per case:
return code 0; the packed, aligned call's bits (query, pack) or the float64 restatement at TOL (scores, gradient rows);
no NaN in the output; guards intact.  Poison makes a wrong kernel fail by value: nothing is arranged to fault."""
import pytest
import torch

from tests.helpers import carve, guarded_out, assert_guard_intact, raw
from tests import analogy_ref as ar

pytestmark = pytest.mark.gpu

TOL = 1e-5
ALL_AT_ONCE = [(0, 0), (1, 0), (3, 0), (4, 0), (8, 0), (0, 1), (0, 2), (0, 3), (1, 1), (3, 2), (4, 3), (8, 1), (4, 2)]
ONE_AT_A_TIME = [(1, 0), (4, 0), (0, 1), (0, 3)]
OUT_PAD = {0: 0, 1: 1, 3: 5, 4: 4, 8: 5}
TABLES = ('sc_e', 're_e', 'im_e', 'sc_r', 're_r', 'im_r')


def layouts():
    out = [dict({o: lay for o in TABLES}, out=(OUT_PAD[lay[0]], lay[1])) for lay in ALL_AT_ONCE]
    for o in TABLES + ('out',):
        for lay in ONE_AT_A_TIME + ([(5, 2)] if o == 'out' else []):
            out.append(dict({x: (0, 0) for x in TABLES + ('out',)}, **{o: lay}))
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def A():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from torchkge_amd import _hip_analogy
    _hip_analogy.load_library()
    return _hip_analogy


@pytest.mark.parametrize('d_sc,d_c', [(3, 4), (16, 16), (9, 23)])
def test_analogy_entry_points_with_carved_operands(A, d_sc, d_c):
    from torchkge_amd import _hip
    lib = A.load_library()
    n_ent, n_rel, B = 60, 5, 80
    K = d_sc + 2 * d_c
    g = torch.Generator().manual_seed(100 * d_sc + d_c)
    tabs = [torch.randn(n, d, generator=g) * 0.5 for n, d in ((n_ent, d_sc), (n_ent, d_c), (n_ent, d_c),
                                                              (n_rel, d_sc), (n_rel, d_c), (n_rel, d_c))]
    h, t, r = [torch.randint(0, n, (B,), generator=g) for n in (n_ent, n_ent, n_rel)]
    go = torch.randn(B, generator=g)
    # packed, aligned calls: the bits every layout must reproduce
    dev = [x.cuda() for x in tabs]
    base_q = A.query(_hip.SIDE_BOTH, dev[:3], dev[3:], h.cuda(), t.cuda(), r.cuda())
    base_rel = A.query(A.SIDE_REL, dev[:3], None, h.cuda(), t.cuda(), None)
    base_p = torch.cat(dev[:3], dim=1)[h.cuda()]
    s64 = ar.sf64(tabs, h, t, r)
    # gradient rows: d/dh = go conj(r) t (the head-side query), d/dt = go h r (the tail-side one), d/dr = go conj(h) t
    g64 = torch.cat([go.double().view(-1, 1) * ar.queries64(tabs, 'head', t=t, r=r),
                     go.double().view(-1, 1) * ar.queries64(tabs, 'tail', h=h, r=r),
                     go.double().view(-1, 1) * ar.queries64(tabs, 'rel', h=h, t=t)])
    for lay in layouts():
        tag = ' '.join('%s %d.%d' % (k, v[0], v[1]) for k, v in sorted(lay.items()) if v != (0, 0)) or 'packed'
        c = {n: carve(x, lay[n][0], lay[n][1], device='cuda') for n, x in zip(TABLES, tabs)}
        d_h, d_t = carve(h, off=1, poison=n_ent, device='cuda'), carve(t, off=1, poison=n_ent, device='cuda')
        d_r, d_go = carve(r, off=1, poison=n_rel, device='cuda'), carve(go, off=lay['out'][1], device='cuda')
        ent = [v for n in TABLES[:3] for v in (c[n], c[n].stride(0))]
        rel = [v for n in TABLES[3:] for v in (c[n], c[n].stride(0))]
        po, oo = lay['out']
        P = guarded_out(B, K, po, oo)
        assert raw(lib, 'kge_analogy_pack_rows', *ent, d_sc, d_c, d_h, B, P, P.stride(0)) == 0, tag
        Q = guarded_out(2 * B, K, po, oo)
        assert raw(lib, 'kge_analogy_query', _hip.SIDE_BOTH, *ent, *rel, d_sc, d_c, d_h, d_t, d_r, B, 0, -1, Q, Q.stride(0)) == 0, tag
        Qr = guarded_out(B, K, po + 1, oo)
        assert raw(lib, 'kge_analogy_query', A.SIDE_REL, *ent, None, 0, None, 0, None, 0, d_sc, d_c, d_h, d_t, None, B, 0, -1,
                   Qr, Qr.stride(0)) == 0, tag
        S = guarded_out(B, None, 0, oo)
        assert raw(lib, 'kge_analogy_score_triples', *ent, *rel, d_sc, d_c, d_h, d_t, d_r, B, S) == 0, tag
        G = guarded_out(3 * B, K, po, oo)
        assert raw(lib, 'kge_analogy_score_triples_bwd', *ent, *rel, d_sc, d_c, d_h, d_t, d_r, B, d_go, G, G.stride(0)) == 0, tag
        torch.cuda.synchronize()
        for k, v in (('P', P), ('Q', Q), ('Qr', Qr), ('S', S), ('G', G)):
            assert not bool(torch.isnan(v).any()), (tag, k)
            assert_guard_intact(v)
        assert torch.equal(bits(P), bits(base_p)), tag
        assert torch.equal(bits(Q), bits(base_q)) and torch.equal(bits(Qr), bits(base_rel)), tag
        assert (S.cpu().double() - s64).abs().max().item() < TOL, tag
        assert (G.cpu().double() - g64).abs().max().item() < TOL, tag
        for v in list(c.values()) + [d_h, d_t, d_r, d_go]:
            assert_guard_intact(v)
