# -*- coding: utf-8 -*-
"""ctypes binding of the triplet-classification entry points of libkge_hip.so (include/kge_hip_triplet.h) and their
tensor-level wrappers.  The symbols live in the library _hip.load_library() returns; their prototypes have a header and
a signature table of their own because include/kge_hip.h and its ABI version do not change for them.

Nothing here synchronises or reads back: the one host read of a triplet classification is the evaluator's."""
import torch

from . import _hip
from ._hip import _vp, _i64, _p, _check, _on, _stream, f32c, i64c, require_cuda

_SIGNATURES = {
    'kge_positional_corrupt': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp],
    'kge_relation_max': [_vp, _vp, _i64, _i64, _vp, _vp, _vp],
    'kge_threshold_count': [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
}
_WS_SIZES = ('kge_positional_ws_elems', 'kge_relation_max_ws_elems')        # int64_t f(int64_t)


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip.bind(_SIGNATURES, _WS_SIZES)


def positional_corrupt(heads, tails, rels, mask_u8, u_h, u_t, fb_h, fb_t, offsets_h, values_h, offsets_t, values_t, n_rel):
    """kge_positional_corrupt: (neg_heads, neg_tails) of one batch.  ``fb_h`` / ``fb_t`` may be None when no relation of
    the two indices is empty."""
    lib = load_library()
    require_cuda(heads, tails, rels, mask_u8, u_h, u_t, fb_h, fb_t, offsets_h, values_h, offsets_t, values_t)
    heads, tails, rels = i64c(heads), i64c(tails), i64c(rels)
    if mask_u8.dtype != torch.uint8 or offsets_h.dtype != torch.int64 or offsets_t.dtype != torch.int64 or \
            values_h.dtype != torch.int32 or values_t.dtype != torch.int32:
        raise RuntimeError('torchkge_amd: positional_corrupt takes a uint8 mask, int64 offsets and int32 values')
    if offsets_h.shape[0] != n_rel + 1 or offsets_t.shape[0] != n_rel + 1:
        raise RuntimeError('torchkge_amd: positional_corrupt takes n_rel + 1 offsets per index')
    u_h, u_t = f32c(u_h), f32c(u_t)
    fb_h = None if fb_h is None else i64c(fb_h)
    fb_t = None if fb_t is None else i64c(fb_t)
    # an all-heads / all-tails batch leaves one side's arrays empty: the entry point still wants a pointer
    u_h, u_t, fb_h, fb_t = (x.new_zeros(1) if x is not None and x.numel() == 0 else x for x in (u_h, u_t, fb_h, fb_t))
    mask_u8, offsets_h, offsets_t = mask_u8.contiguous(), offsets_h.contiguous(), offsets_t.contiguous()
    values_h, values_t = values_h.contiguous(), values_t.contiguous()
    B, dev = heads.shape[0], heads.device
    nh = torch.empty(B, dtype=torch.int64, device=dev)
    nt = torch.empty(B, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.kge_positional_ws_elems(B)), 1), dtype=torch.int32, device=dev)
    with _on(dev):
        _check(lib.kge_positional_corrupt(_p(heads), _p(tails), _p(rels), _p(mask_u8), _p(u_h), _p(u_t), _p(fb_h), _p(fb_t),
                                          _p(offsets_h), _p(values_h), _p(offsets_t), _p(values_t), n_rel, B, _p(nh), _p(nt),
                                          _p(ws), _stream()), 'kge_positional_corrupt')
    return nh, nt


def relation_max(scores, rels, n_rel):
    """kge_relation_max: fp32 (n_rel) thresholds; all NaN for an empty score vector (the maximum of nothing)."""
    lib = load_library()
    require_cuda(scores, rels)
    scores, rels = f32c(scores), i64c(rels)
    n, dev = scores.shape[0], scores.device
    if rels.shape[0] != n:
        raise RuntimeError('torchkge_amd: relation_max takes one relation per score')
    thr = torch.full((n_rel,), float('nan'), dtype=torch.float32, device=dev) if n == 0 else \
        torch.empty(n_rel, dtype=torch.float32, device=dev)
    ws = torch.empty(max(int(lib.kge_relation_max_ws_elems(n_rel)), 1), dtype=torch.int32, device=dev)
    with _on(dev):
        _check(lib.kge_relation_max(_p(scores), _p(rels), n, n_rel, _p(thr), _p(ws), _stream()), 'kge_relation_max')
    return thr


def threshold_count(pos, neg, rels, thr):
    """kge_threshold_count: int64 (2) device tensor [#{pos > thr[rels]}, #{neg < thr[rels]}]."""
    lib = load_library()
    require_cuda(pos, neg, rels, thr)
    pos, neg, rels, thr = f32c(pos), f32c(neg), i64c(rels), f32c(thr)
    n, dev = pos.shape[0], pos.device
    if neg.shape[0] != n or rels.shape[0] != n:
        raise RuntimeError('torchkge_amd: threshold_count takes vectors of one length')
    counts = torch.zeros(2, dtype=torch.int64, device=dev) if n == 0 else torch.empty(2, dtype=torch.int64, device=dev)
    with _on(dev):
        _check(lib.kge_threshold_count(_p(pos), _p(neg), _p(rels), _p(thr), n, thr.shape[0], _p(counts), _stream()),
               'kge_threshold_count')
    return counts
