# -*- coding: utf-8 -*-
"""ctypes binding of include/kge_hip_rotate.h: the query rows of RotatE.  The mode KGE_LP_CMOD and the kind KGE_ROTATE of
that header are ``_hip.LP_CMOD`` / ``_hip.ROTATE``; they go through the entry points of include/kge_hip.h."""
import torch

from . import _hip
from ._hip import _vp, _i64, _int, _p, _check, _on, _stream

_SIGNATURES = {
    'kge_rotate_query': [_int, _vp, _i64, _vp, _i64, _int, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp],
}
EXPORTED_SYMBOLS = sorted(_SIGNATURES)


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip.bind(_SIGNATURES)


def rotate_query(side, E, P, h, t, r, ent_lo=0, ent_n=-1):
    """kge_rotate_query: the (B, 2d) -- side SIDE_BOTH: (2B, 2d) -- interleaved query rows of RotatE, E[h] o r (tail side)
    or E[t] o conj(r) (head side).  ent_n >= 0: E holds only the rows [ent_lo, ent_lo + ent_n), rows of other entities
    come back as zeros (to be summed over the shards)."""
    _hip.require_cuda(E, P, h, t, r)
    lib = load_library()
    E, P = _hip.f32rows(E), _hip.f32rows(P)
    h, t, r = _hip.i64c(h), _hip.i64c(t), _hip.i64c(r)
    d, B = P.shape[1], r.shape[0]
    if E.shape[1] != 2 * d:
        raise RuntimeError('torchkge_amd: rotate_query needs entity rows of 2 * %d floats, got %d' % (d, E.shape[1]))
    rows = 2 * B if side == _hip.SIDE_BOTH else B
    Q = torch.empty(rows, 2 * d, dtype=torch.float32, device=E.device)
    if rows:
        with _on(E.device):
            _check(lib.kge_rotate_query(side, _p(E), E.stride(0), _p(P), P.stride(0), d, _p(h), _p(t), _p(r), B, ent_lo,
                                        ent_n, _p(Q), Q.stride(0), _stream()), 'kge_rotate_query')
    return Q
