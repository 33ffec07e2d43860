# -*- coding: utf-8 -*-
"""ctypes binding of the deterministic reduction of libkge_hip.so (include/kge_hip_det.h) and the one place where a
backward chooses its row reduction: ``segment_sum`` calls kge_segment_sum_rows (atomic row-adds per run) or
kge_segment_sum_ordered (one writer per row, fixed order) by torchkge_amd.determinism.is_deterministic().

The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature table of
their own because include/kge_hip.h and its ABI version do not change for them.  Nothing here synchronises or reads
back."""
import ctypes

import torch

from . import _hip
from ._hip import _vp, _i64, _int, _check, _on, _stream
from .determinism import is_deterministic

_size = ctypes.c_size_t
_SIGNATURES = {
    'kge_segment_sum_ordered': [_vp, _i64, _int, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _size, _vp],
}
_WS_SIZES = ('kge_segment_sum_ordered_ws_bytes',)       # size_t f(int64_t M, int d)
_WS_BYTES = {}      # (M, d) -> workspace bytes
SEG_MAX = 1024      # widest row one kge_segment_sum_rows / kge_segment_sum_ordered call reduces
# how often each reduction was launched by segment_sum / segment_sum_ordered (tests read it: which path a backward took)
CALLS = {'ordered': 0, 'atomic': 0}


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip.bind(_SIGNATURES, _WS_SIZES, (_i64, _int), _size)


def ws_bytes(M, d):
    """kge_segment_sum_ordered_ws_bytes: host arithmetic, cached per (M, d)."""
    nb = _WS_BYTES.get((M, d))
    if nb is None:
        nb = _WS_BYTES[(M, d)] = int(load_library().kge_segment_sum_ordered_ws_bytes(M, d))
    return nb


def _ptr(x):
    """A tensor's data pointer, or an address (a view into a larger buffer: base + byte offset), or None."""
    return x if x is None or x.__class__ is int else x.data_ptr()


def segment_sum_ordered(rows, ld, d, k0, n0, k1, n1, perm, out, out_ld, ws=None):
    """kge_segment_sum_ordered on the current stream: out[key, :d] += the rows of each key of [k0 | k1], summed in a
    fixed order without float atomics.  ``rows`` / ``out``: tensors or device addresses; ``perm``: the stable ascending
    order of the keys (a tensor: its device is the launch's).  ``ws``: a uint8 workspace of at least ws_bytes(n0 + n1, d)
    bytes; None allocates one."""
    lib = load_library()
    M = n0 + n1
    nb = ws_bytes(M, d) if 1 <= d <= 1024 and M > 0 else 0
    if ws is None:
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=perm.device)
    CALLS['ordered'] += 1
    with _on(perm.device):
        _check(lib.kge_segment_sum_ordered(_ptr(rows), ld, d, _ptr(k0), n0, _ptr(k1), n1, _ptr(perm), _ptr(out), out_ld,
                                           _ptr(ws), ws.numel(), _stream()), 'kge_segment_sum_ordered')


def segment_sum(rows, ld, d, k0, n0, k1, n1, perm, out, out_ld, det=None):
    """The row reduction of every backward: kge_segment_sum_rows, or kge_segment_sum_ordered in deterministic mode
    (``det``: the mode as the caller has already read it; None asks).  The caller has made ``perm``'s device current."""
    if is_deterministic() if det is None else det:
        return segment_sum_ordered(rows, ld, d, k0, n0, k1, n1, perm, out, out_ld)
    CALLS['atomic'] += 1
    rc = (_hip._lib or _hip.load_library()).kge_segment_sum_rows(_ptr(rows), ld, d, _ptr(k0), n0, _ptr(k1), n1, _ptr(perm), _ptr(out), out_ld, _stream())
    if rc:
        _check(rc, 'kge_segment_sum_rows')


def reduce_rows(rows, ld, d, k0, k1, out, out_ld=None, perm=None, det=None):
    """The end of every backward: out[id, :d] += the rows (leading dimension ``ld``) of each id of [k0 | k1] (``k1`` may be
    None), through segment_sum.  ``rows`` / ``out``: tensors or device addresses; ``out_ld``: None takes out.stride(0).
    ``perm``: the ids' sorted order; None sorts them here (_hip._key_perm: the ids index the out.shape[0] rows of the
    tensor ``out``).  Returns the order, for the caller to pass back in when it reduces another table by the same ids: one
    sort per id set and backward.  Rows wider than SEG_MAX go in column chunks.  ``det``: the mode as the backward has
    read it, once.  An empty id list launches nothing (the library returns before any launch); the caller has made the
    ids' device current."""
    n0, n1 = k0.shape[0], (0 if k1 is None else k1.shape[0])
    if perm is None:
        perm = _hip._key_perm(k0, k1, max(out.shape[0], 1))
    if out_ld is None:
        out_ld = out.stride(0)
    if det is None:
        det = is_deterministic()
    rows, out = _ptr(rows), _ptr(out)
    for c0 in range(0, d, SEG_MAX):
        segment_sum(rows + 4 * c0, ld, min(SEG_MAX, d - c0), k0, n0, k1, n1, perm, out + 4 * c0, out_ld, det)
    return perm
