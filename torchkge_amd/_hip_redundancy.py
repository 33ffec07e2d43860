# -*- coding: utf-8 -*-
"""ctypes binding of the data-redundancy entry points of libkge_hip.so (include/kge_hip_redundancy.h) and their
tensor-level wrappers.  The symbols live in the library _hip.load_library() returns; their prototypes have a header and a
signature table of their own because include/kge_hip.h and its ABI version do not change for them.

Nothing here synchronises or reads back."""
import ctypes

import torch

from . import _hip
from ._hip import _vp, _i64, _p, _check, _on, _stream, i64c, require_cuda

_f64 = ctypes.c_double

_SIGNATURES = {
    'kge_relation_overlap': [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _vp],
    'kge_relation_stats': [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp],
    'kge_overlap_select': [_vp, _i64, _vp, _i64, _f64, _f64, _vp, _i64, _vp, _vp, _i64, _vp],
}
_WS_SIZES = ('kge_relation_stats_ws_bytes', 'kge_overlap_select_ws_bytes')      # int64_t f(int64_t)
_WS_SIZES_2 = ('kge_relation_overlap_ws_bytes',)                                # int64_t f(int64_t, int64_t)
_SIGNATURES_2 = {}      # (the key of _hip.bind's once-per-handle cache for the two-argument size query)

KGE_EUNSUPPORTED = -3


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    _hip.bind(_SIGNATURES_2, _WS_SIZES_2, size_argtypes=(_i64, _i64))
    return _hip.bind(_SIGNATURES, _WS_SIZES)


def _ws(n_bytes, dev):
    return torch.empty(max(int(n_bytes), 1), dtype=torch.uint8, device=dev)


def relation_overlap(a, b, n_ent, n_rel, want_rev=True):
    """kge_relation_overlap: (same, rev) int32 (n_rel, n_rel) of the fact lists ``a`` = (h, t, r) and ``b`` (None: B = A);
    rev is None when ``want_rev`` is false."""
    lib = load_library()
    a = tuple(i64c(x) for x in a)
    b = None if b is None else tuple(i64c(x) for x in b)
    require_cuda(*(a + (b or ())))
    dev = a[0].device
    n_a, n_b = a[0].shape[0], (0 if b is None else b[0].shape[0])
    if any(x.shape[0] != n_a for x in a) or (b is not None and any(x.shape[0] != n_b for x in b)):
        raise RuntimeError('torchkge_amd: relation_overlap takes heads, tails and relations of one length')
    same = torch.empty(n_rel, n_rel, dtype=torch.int32, device=dev)
    rev = torch.empty(n_rel, n_rel, dtype=torch.int32, device=dev) if want_rev else None
    ws_bytes = int(lib.kge_relation_overlap_ws_bytes(n_a, n_b))
    ws = _ws(ws_bytes, dev)
    if b is None:
        pb = (None, None, None)
    else:       # an EMPTY B is not "B = A": it keeps a non-NULL pointer
        pb = tuple(_p(x) if n_b else _p(ws) for x in b)
    with _on(dev):
        rc = lib.kge_relation_overlap(_p(a[0]), _p(a[1]), _p(a[2]), n_a, pb[0], pb[1], pb[2], n_b, n_ent, n_rel,
                                      _p(same), _p(rev), n_rel, _p(ws), ws_bytes, _stream())
    if rc == KGE_EUNSUPPORTED:
        raise RuntimeError('torchkge_amd: relation_overlap packs (pair, orientation, set, relation) into 64 bits; '
                           'n_ent = %d with n_rel = %d needs more' % (n_ent, n_rel))
    _check(rc, 'kge_relation_overlap')
    return same, rev


def relation_stats(h, t, r, n_ent, n_rel):
    """kge_relation_stats: int64 (3, n_rel) -- facts with repeats, distinct heads, distinct tails per relation."""
    lib = load_library()
    h, t, r = i64c(h), i64c(t), i64c(r)
    require_cuda(h, t, r)
    dev, n = h.device, h.shape[0]
    out = torch.empty(3, n_rel, dtype=torch.int64, device=dev)
    ws_bytes = int(lib.kge_relation_stats_ws_bytes(n))
    ws = _ws(ws_bytes, dev)
    with _on(dev):
        _check(lib.kge_relation_stats(_p(h), _p(t), _p(r), n, n_ent, n_rel, _p(out), _p(ws), ws_bytes, _stream()),
               'kge_relation_stats')
    return out


def overlap_select(counts, lengths, theta1, theta2, pairs, n_out):
    """kge_overlap_select into the caller's ``pairs`` (int32 (cap, 2), contiguous) and ``n_out`` (one int64)."""
    lib = load_library()
    require_cuda(counts, lengths, pairs, n_out)
    n_rel = counts.shape[0]
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.stride(1) != 1 or lengths.dtype != torch.int64 or \
            pairs.dtype != torch.int32 or not pairs.is_contiguous() or n_out.dtype != torch.int64:
        raise RuntimeError('torchkge_amd: overlap_select takes int32 counts and pairs, int64 lengths and n_out')
    ws_bytes = int(lib.kge_overlap_select_ws_bytes(n_rel))
    ws = _ws(ws_bytes, counts.device)
    with _on(counts.device):
        _check(lib.kge_overlap_select(_p(counts), counts.stride(0), _p(lengths.contiguous()), n_rel, float(theta1), float(theta2),
                                      _p(pairs), pairs.shape[0], _p(n_out), _p(ws), ws_bytes, _stream()),
               'kge_overlap_select')
