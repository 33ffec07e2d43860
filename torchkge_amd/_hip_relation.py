# -*- coding: utf-8 -*-
"""ctypes binding of the relation-side entry point of libkge_hip.so (include/kge_hip_relation.h) and its tensor-level
wrapper.  The symbol lives in the library _hip.load_library() returns; its prototype has a header and a signature table
of its own because include/kge_hip.h and its ABI version do not change for it.

Nothing here synchronises or reads back."""
import torch

from . import _hip
from ._hip import _vp, _i64, _p, _check, _on, _stream, i64c, require_cuda

_SIGNATURES = {
    'kge_relation_corrupt': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
}
_WS_SIZES = ('kge_relation_corrupt_ws_elems',)        # int64_t f(int64_t)


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip.bind(_SIGNATURES, _WS_SIZES)


def _u8c(t, what):
    if t is None:
        return None
    if t.dtype != torch.uint8:
        raise RuntimeError('torchkge_amd: relation_corrupt takes uint8 masks (%s is %s)' % (what, t.dtype))
    return t.contiguous()


def relation_corrupt(heads, tails, rels, mask_ent, mask_head, draws_r, draws_h, draws_t, n_neg=1):
    """kge_relation_corrupt: (neg_heads, neg_tails, neg_rels), int64 (B * n_neg), of one batch of B facts.  ``mask_ent``
    is uint8 (B * n_neg); ``mask_head`` is uint8 and compact (one byte per non-zero ``mask_ent`` byte, or longer).
    ``mask_head`` and the three draw arrays may be None or empty when their branch cannot be taken."""
    lib = load_library()
    require_cuda(heads, tails, rels, mask_ent, mask_head, draws_r, draws_h, draws_t)
    heads, tails, rels = i64c(heads), i64c(tails), i64c(rels)
    B, dev = heads.shape[0], heads.device
    n = B * n_neg
    if tails.shape[0] != B or rels.shape[0] != B:
        raise RuntimeError('torchkge_amd: relation_corrupt takes heads, tails and relations of one length')
    mask_ent, mask_head = _u8c(mask_ent, 'mask_ent'), _u8c(mask_head, 'mask_head')
    if mask_ent.shape[0] != n:
        raise RuntimeError('torchkge_amd: relation_corrupt takes one mask_ent byte per position (B * n_neg)')
    # an empty tensor becomes a NULL pointer: the entry point never dereferences the array of a branch that is not taken
    mask_head, draws_r, draws_h, draws_t = (None if x is None or x.numel() == 0 else x
                                            for x in (mask_head, draws_r, draws_h, draws_t))
    draws_r, draws_h, draws_t = (None if x is None else i64c(x) for x in (draws_r, draws_h, draws_t))
    nh = torch.empty(n, dtype=torch.int64, device=dev)
    nt = torch.empty(n, dtype=torch.int64, device=dev)
    nr = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.kge_relation_corrupt_ws_elems(n)), 1), dtype=torch.int32, device=dev)
    with _on(dev):
        _check(lib.kge_relation_corrupt(_p(heads), _p(tails), _p(rels), _p(mask_ent), _p(mask_head), _p(draws_r), _p(draws_h),
                                        _p(draws_t), B, n_neg, _p(nh), _p(nt), _p(nr), _p(ws), _stream()),
               'kge_relation_corrupt')
    return nh, nt, nr
