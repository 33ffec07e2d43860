# -*- coding: utf-8 -*-
"""ctypes binding of the ANALOGY entry points of libkge_hip.so (include/kge_hip_analogy.h) and their tensor-level
wrappers.  The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature
table of their own because include/kge_hip.h, kge_lp_desc and its ABI version do not change for this model."""
import torch

from . import _hip, _hip_det
from ._hip_rows import sparse_rows
from ._hip import _vp, _i64, _int, _p, _check, _on, _stream, f32c, f32rows, i64c, require_cuda

SIDE_REL = 5        # KGE_ANALOGY_SIDE_REL
MAX_DIM = 512       # of each of d_sc, d_c

_T3 = [_vp, _i64, _vp, _i64, _vp, _i64]     # three tables (sc, re, im), each with its leading dimension
_SIGNATURES = {
    'kge_analogy_pack_rows': _T3 + [_int, _int, _vp, _i64, _vp, _i64, _vp],
    'kge_analogy_query': [_int] + _T3 + _T3 + [_int, _int, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp],
    'kge_analogy_score_triples': _T3 + _T3 + [_int, _int, _vp, _vp, _vp, _i64, _vp, _vp],
    'kge_analogy_score_triples_bwd': _T3 + _T3 + [_int, _int, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp],
}


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip.bind(_SIGNATURES)


def _t3(tabs):
    """(pointer, leading dimension) x 3 of a (sc, re, im) triple; a zero-width table passes NULL, 0."""
    out = []
    for x in tabs:
        if x is None or x.shape[1] == 0:
            out += [None, 0]
        else:
            out += [_p(x), x.stride(0)]
    return out


def _prep(tabs):
    tabs = [None if x is None else f32rows(x) for x in tabs]
    require_cuda(*tabs)
    return tabs


def _dims(tabs):
    return int(tabs[0].shape[1]), int(tabs[1].shape[1])


def pack_rows(tabs, idx=None):
    """kge_analogy_pack_rows: packed rows [sc | re | im] of the three tables ``tabs`` -- all of them, or those of
    ``idx``.  Returns a (rows, K rounded up to 4) matrix whose first K columns are the packed row and whose pad
    columns are zero: the leading dimension lets the DOT operand builders take their aligned bodies (the problem's
    width stays K: kge_lp_desc.K0)."""
    lib = load_library()
    tabs = _prep(tabs)
    d_sc, d_c = _dims(tabs)
    K = d_sc + 2 * d_c
    idx = None if idx is None else i64c(idx)
    require_cuda(idx)
    rows = tabs[0].shape[0] if idx is None else idx.shape[0]
    K4 = (K + 3) // 4 * 4
    out = (torch.empty if K4 == K else torch.zeros)(rows, K4, dtype=torch.float32, device=tabs[0].device)
    if rows:
        with _on(out.device):
            _check(lib.kge_analogy_pack_rows(*(_t3(tabs) + [d_sc, d_c, _p(idx), rows, _p(out), K4, _stream()])),
                   'kge_analogy_pack_rows')
    return out


def query(side, ent, rel, h, t, r, B=None, ent_lo=0, ent_n=-1):
    """kge_analogy_query: the (B, K) -- side 'both': (2B, K) -- query rows.  ``ent`` / ``rel``: (sc, re, im) triples;
    h = t = r = None: already-gathered rows (``B`` rows; SIDE_REL: ``rel`` holds the tails' rows)."""
    lib = load_library()
    ent = _prep(ent)
    rel = [None] * 3 if rel is None else _prep(rel)
    d_sc, d_c = _dims(ent)
    h, t, r = (None if x is None else i64c(x) for x in (h, t, r))
    require_cuda(h, t, r)
    if B is None:
        B = next(x for x in (r, h, t) if x is not None).shape[0]
    rows = 2 * B if side == _hip.SIDE_BOTH else B
    Q = torch.empty(rows, d_sc + 2 * d_c, dtype=torch.float32, device=ent[0].device)
    if rows:
        with _on(Q.device):
            _check(lib.kge_analogy_query(*([side] + _t3(ent) + _t3(rel) + [d_sc, d_c, _p(h), _p(t), _p(r), B, ent_lo, ent_n,
                                                                            _p(Q), Q.stride(0), _stream()])),
                   'kge_analogy_query')
    return Q


def score_triples(ent, rel, h, t, r):
    lib = load_library()
    ent, rel = _prep(ent), _prep(rel)
    d_sc, d_c = _dims(ent)
    h, t, r = i64c(h), i64c(t), i64c(r)
    require_cuda(h, t, r)
    B = h.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=h.device)
    with _on(h.device):
        _check(lib.kge_analogy_score_triples(*(_t3(ent) + _t3(rel) + [d_sc, d_c, _p(h), _p(t), _p(r), B, _p(out), _stream()])),
               'kge_analogy_score_triples')
    return out


def score_triples_bwd(ent, rel, h, t, r, grad_out, needs, row_grads=False):
    """Gradients of the six tables (None where ``needs`` says so): per-triple gradient rows in packed layout, reduced
    per entity / relation by _hip_det.reduce_rows (kge_key_sort, then kge_segment_sum_rows, or kge_segment_sum_ordered in
    deterministic mode) into packed gradients whose column slices are the tables' -- no per-element atomics.
    ``row_grads`` (torchkge_amd.rowgrad, as the forward read it): no reduction -- every gradient is the uncoalesced sparse
    tensor of the ids and a copy of its column slice of the packed rows."""
    lib = load_library()
    ent, rel = _prep(ent), _prep(rel)
    d_sc, d_c = _dims(ent)
    K = d_sc + 2 * d_c
    h, t, r = i64c(h), i64c(t), i64c(r)
    go = f32c(grad_out)
    B, dev = h.shape[0], h.device
    n_ent, n_rel = ent[0].shape[0], rel[0].shape[0]
    rows = torch.empty(3 * B, K, dtype=torch.float32, device=dev)
    out = [None] * 6
    det = _hip_det.is_deterministic()
    with _on(dev):
        _check(lib.kge_analogy_score_triples_bwd(*(_t3(ent) + _t3(rel) + [d_sc, d_c, _p(h), _p(t), _p(r), B, _p(go), _p(rows),
                                                                           K, _stream()])), 'kge_analogy_score_triples_bwd')
        for first, n_rows, k0, k1, src in ((0, n_ent, h, t, rows), (3, n_rel, r, None, rows[2 * B:])):
            if not any(needs[first:first + 3]):
                continue
            if row_grads:
                ids = r if k1 is None else torch.cat((k0, k1))
                for j, (c0, c1) in enumerate(((0, d_sc), (d_sc, d_sc + d_c), (d_sc + d_c, K))):
                    if needs[first + j]:
                        out[first + j] = sparse_rows(ids, src[:ids.shape[0], c0:c1].contiguous(), (n_rows, c1 - c0))
                continue
            g = torch.zeros(n_rows, K, dtype=torch.float32, device=dev)
            if B:
                _hip_det.reduce_rows(src, K, K, k0, k1, g, det=det)
            parts = (g[:, :d_sc], g[:, d_sc:d_sc + d_c], g[:, d_sc + d_c:])
            for j in range(3):
                out[first + j] = parts[j] if needs[first + j] else None
    return out
