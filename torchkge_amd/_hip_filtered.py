# -*- coding: utf-8 -*-
"""ctypes binding of the filtered-sampling entries of libkge_hip.so (include/kge_hip_filtered.h) and their tensor-level
wrappers: ``filtered_corrupt`` -- the replacement of a fact's head or tail drawn exactly over the entities that are
neither known answers of its key nor the replaced entity, one kge_filtered_corrupt per batch -- and ``triples_known`` --
which triples are in an index (kge_triples_known).

The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature table of
their own because include/kge_hip.h and its ABI version do not change for them.  Nothing here synchronises or reads
back."""
import torch

from . import _hip
from ._hip import _vp, _i64, _p, _check, _on, _stream, i64c, require_cuda

_SIGNATURES = {
    'kge_filtered_corrupt': [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp],
    'kge_triples_known': [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp],
}


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip.bind(_SIGNATURES)


def _i32c(t, what):
    if t.dtype != torch.int32:
        raise RuntimeError('torchkge_amd: %s is int32 (the targets of a FilterIndex), got %s' % (what, t.dtype))
    return t.contiguous()


def filtered_corrupt(heads, tails, mask, draws, tail_lo, tail_hi, tail_targets, head_lo, head_hi, head_targets, n_ent,
                     n_neg=1, want_exhausted=False):
    """kge_filtered_corrupt on the current stream: ``(neg_heads, neg_tails, exhausted)`` of one batch of B facts -- int64
    (B * n_neg) in tile order (negative k of fact i at k * B + i) and the uint8 flags, or None without
    ``want_exhausted`` (the entry then gets a NULL pointer).  ``mask`` is uint8 (B * n_neg), 1 = replace the head;
    ``draws`` int64 (B * n_neg), any bit pattern; the four bounds are int64 (B), the two target arrays int32."""
    lib = load_library()
    require_cuda(heads, tails, mask, draws, tail_lo, tail_hi, tail_targets, head_lo, head_hi, head_targets)
    heads, tails, draws = i64c(heads), i64c(tails), i64c(draws)
    tail_lo, tail_hi, head_lo, head_hi = (i64c(x) for x in (tail_lo, tail_hi, head_lo, head_hi))
    tail_targets, head_targets = _i32c(tail_targets, 'tail_targets'), _i32c(head_targets, 'head_targets')
    B, dev = heads.shape[0], heads.device
    n = B * n_neg
    if mask.dtype != torch.uint8:
        raise RuntimeError('torchkge_amd: filtered_corrupt takes a uint8 mask (got %s)' % mask.dtype)
    mask = mask.contiguous()
    if tails.shape[0] != B or any(x.shape[0] != B for x in (tail_lo, tail_hi, head_lo, head_hi)):
        raise RuntimeError('torchkge_amd: filtered_corrupt takes heads, tails and the four bounds of one length')
    if mask.shape[0] != n or draws.shape[0] != n:
        raise RuntimeError('torchkge_amd: filtered_corrupt takes one mask byte and one draw per position (B * n_neg)')
    nh = torch.empty(n, dtype=torch.int64, device=dev)
    nt = torch.empty(n, dtype=torch.int64, device=dev)
    ex = torch.empty(n, dtype=torch.uint8, device=dev) if want_exhausted else None
    with _on(dev):
        _check(lib.kge_filtered_corrupt(_p(heads), _p(tails), B, n_neg, _p(mask), _p(draws), _p(tail_lo), _p(tail_hi),
                                        _p(tail_targets), _p(head_lo), _p(head_hi), _p(head_targets), n_ent, _p(nh),
                                        _p(nt), _p(ex), _stream()), 'kge_filtered_corrupt')
    return nh, nt, ex


def triples_known(keys, offsets, targets, key_span, key1, key2, value):
    """kge_triples_known on the current stream: uint8 (n), 1 where ``value[p]`` is in the list of ``(key1[p], key2[p])``
    of the index ``(keys, offsets, targets)``."""
    lib = load_library()
    require_cuda(keys, offsets, targets, key1, key2, value)
    key1, key2, value = i64c(key1), i64c(key2), i64c(value)
    n = key1.shape[0]
    if key2.shape[0] != n or value.shape[0] != n:
        raise RuntimeError('torchkge_amd: triples_known takes three id vectors of one length')
    keys, offsets, targets = i64c(keys), i64c(offsets), _i32c(targets, 'targets')
    out = torch.empty(n, dtype=torch.uint8, device=key1.device)
    with _on(key1.device):
        _check(lib.kge_triples_known(_p(keys), keys.shape[0], _p(offsets), _p(targets), key_span, _p(key1), _p(key2),
                                     _p(value), n, _p(out), _stream()), 'kge_triples_known')
    return out
