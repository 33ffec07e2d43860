# -*- coding: utf-8 -*-
"""ctypes binding of the row-gradient entries of libkge_hip.so (include/kge_hip_rows.h): kge_rows_coalesce and the row
updates kge_row_sgd / kge_row_adagrad / kge_row_adam, and the helper every backward uses to hand out a table's gradient
as an uncoalesced sparse tensor (``sparse_rows``).

The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature table of
their own because include/kge_hip.h and its ABI version do not change for them.  Nothing here synchronises or reads
back."""
import ctypes

import torch

from . import _hip
from ._hip import _vp, _i64, _int, _check, _on, _p, _stream

_size = ctypes.c_size_t
_f32 = ctypes.c_float
_SIGNATURES = {
    'kge_rows_coalesce': [_vp, _i64, _int, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _size, _vp],
    'kge_row_sgd': [_vp, _i64, _int, _vp, _vp, _i64, _vp, _i64, _f32, _vp],
    'kge_row_adagrad': [_vp, _vp, _i64, _int, _vp, _vp, _i64, _vp, _i64, _f32, _f32, _vp],
    'kge_row_adam': [_vp, _vp, _vp, _i64, _int, _vp, _vp, _i64, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _f32, _vp],
}
_WS_SIZES = ('kge_rows_coalesce_ws_bytes',)     # size_t f(int64_t M, int d)
_WS_BYTES = {}      # (M, d) -> workspace bytes


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    lib = _hip.bind(_SIGNATURES, _WS_SIZES, (_i64, _int), _size)
    lib.kge_row_update_max_waves.argtypes, lib.kge_row_update_max_waves.restype = [], _int
    return lib


def ws_bytes(M, d):
    """kge_rows_coalesce_ws_bytes, cached per (M, d)."""
    nb = _WS_BYTES.get((M, d))
    if nb is None:
        nb = _WS_BYTES[(M, d)] = int(load_library().kge_rows_coalesce_ws_bytes(M, d))
    return nb


def max_waves():
    """kge_row_update_max_waves: the grid cap of the row updates, in wavefronts."""
    return int(load_library().kge_row_update_max_waves())


def sparse_rows(ids, values, shape):
    """The gradient of a ``shape`` table as an uncoalesced sparse COO tensor: row ids[i] gets values[i] (ids repeat).
    No sort, no sum, no table-sized tensor; the tensors are used as they are (``values`` may be a view)."""
    return torch.sparse_coo_tensor(ids.view(1, -1), values, tuple(shape), check_invariants=False)


def rows_coalesce(rows, ld, d, ids, n_rows, uniq=None, out=None, out_ld=None, count=None):
    """kge_rows_coalesce on the current stream: (uniq, out, count) -- the distinct ids ascending, their summed rows
    (compact: row j belongs to uniq[j]) and their number as a device int64 scalar.  ``rows``: a float32 tensor whose M
    rows lie ``ld`` floats apart; ``ids``: M contiguous int64.  The outputs have room for M; only the first ``count`` of
    each mean anything."""
    lib = load_library()
    M, dev = ids.shape[0], ids.device
    if uniq is None:
        uniq = torch.empty(M, dtype=torch.int64, device=dev)
    if out is None:
        out, out_ld = torch.empty(M, d, dtype=torch.float32, device=dev), d
    if count is None:
        count = torch.empty((), dtype=torch.int64, device=dev)
    nb = ws_bytes(M, d) if M > 0 else 0
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    with _on(dev):
        _check(lib.kge_rows_coalesce(_p(rows), ld, d, _p(ids), M, n_rows, _p(uniq), _p(out), out_ld, _p(count), _p(ws),
                                     ws.numel(), _stream()), 'kge_rows_coalesce')
    return uniq, out, count


def row_sgd(p, uniq, count, g, lr):
    """kge_row_sgd: p[uniq[j]] -= lr * g[j] for j < count."""
    with _on(p.device):
        _check(load_library().kge_row_sgd(_p(p), p.stride(0), p.shape[1], _p(uniq), _p(count), uniq.shape[0], _p(g),
                                          g.stride(0), lr, _stream()), 'kge_row_sgd')


def row_adagrad(p, state_sum, uniq, count, g, clr, eps):
    """kge_row_adagrad on the rows uniq[j], j < count, of ``p`` and ``state_sum`` (same layout)."""
    with _on(p.device):
        _check(load_library().kge_row_adagrad(_p(p), _p(state_sum), p.stride(0), p.shape[1], _p(uniq), _p(count),
                                              uniq.shape[0], _p(g), g.stride(0), clr, eps, _stream()), 'kge_row_adagrad')


def row_adam(p, exp_avg, exp_avg_sq, uniq, count, g, lr, beta1, beta2, eps, step):
    """kge_row_adam (SparseAdam's lazy update) on the rows uniq[j], j < count; ``step``: the global step, from 1.  The
    complements 1 - beta and the bias corrections 1 - beta ** step are taken here in double precision."""
    with _on(p.device):
        _check(load_library().kge_row_adam(_p(p), _p(exp_avg), _p(exp_avg_sq), p.stride(0), p.shape[1], _p(uniq), _p(count),
                                           uniq.shape[0], _p(g), g.stride(0), lr, 1 - beta1, 1 - beta2, eps,
                                           1 - beta1 ** step, 1 - beta2 ** step, _stream()), 'kge_row_adam')
