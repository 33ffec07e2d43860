# -*- coding: utf-8 -*-
"""ctypes binding of the embedding regularizers of libkge_hip.so (include/kge_hip_penalty.h): ``row_penalty`` -- the Lp
penalty of the table rows a batch names, summed in a fixed order -- ``row_penalty_bwd`` -- its gradient rows, one per
occurrence -- and the ``torch.autograd.Function`` around the two (``RowPenalty``), whose backward reduces the rows into
dense tables through _hip_det.reduce_rows or, inside ``row_gradients()``, hands them on as uncoalesced sparse gradients.

The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature table of
their own because include/kge_hip.h and its ABI version do not change for them.  Nothing here synchronises or reads
back."""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _hip, _hip_det
from ._hip import _vp, _i64, _int, _check, _on, _p, _stream, i64c

_size = ctypes.c_size_t
_SIGNATURES = {
    'kge_row_penalty': [_vp, _int, _int, _vp, _vp, _vp, _vp, _size, _vp],
    'kge_row_penalty_bwd': [_vp, _int, _int, _vp, _vp, _vp],
}
# the host arithmetic of the header: name -> (argtypes, restype)
_QUERIES = {
    'kge_row_penalty_terms': ([_vp, _int], _i64),
    'kge_row_penalty_ws_bytes': ([_i64], _size),
    'kge_row_penalty_rows_floats': ([_vp, _int], _i64),
    'kge_row_penalty_row_offset': ([_vp, _int, _int], _i64),
}
REAL, SPLIT, INTERLEAVED = 0, 1, 2              # KGE_PENALTY_* of the header
MAX_STREAMS, WAVES, MAX_BLOCKS = 8, 4, 2048     # KGE_PENALTY_MAX_STREAMS, _WAVES, _MAX_BLOCKS


class PenaltyStream(ctypes.Structure):
    """kge_penalty_stream."""
    _fields_ = [('t0', _vp), ('t1', _vp), ('ld', _i64), ('d', _int), ('layout', _int), ('ids', _vp), ('n', _i64),
                ('factor', ctypes.c_float)]


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    lib = _hip.bind(_SIGNATURES)
    for name, (args, res) in _QUERIES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, res
    return lib


def _rows(t):
    """A float32 table whose rows are contiguous (its row stride is the stream's leading dimension)."""
    return _hip.f32rows(t)


def descriptors(streams):
    """(ctypes array of kge_penalty_stream, the tensors it points into) of ``streams``: tuples ``(layout, t0, t1, ids,
    factor)`` with ``t1`` None unless the layout is SPLIT.  The width d is the tables' second dimension."""
    arr = (PenaltyStream * max(len(streams), 1))()
    keep = []
    for q, (layout, t0, t1, ids, factor) in enumerate(streams):
        t0, t1, ids = _rows(t0), (None if t1 is None else _rows(t1)), i64c(ids)
        if t1 is not None:
            if t1.shape != t0.shape:
                raise ValueError('torchkge_amd: the two tables of a SPLIT stream have the shapes %s and %s'
                                 % (tuple(t0.shape), tuple(t1.shape)))
            if t1.stride(0) != t0.stride(0):
                t0, t1 = t0.contiguous(), t1.contiguous()       # a SPLIT pair shares one leading dimension
        keep += [t0, t1, ids]
        arr[q] = PenaltyStream(t0.data_ptr(), None if t1 is None else t1.data_ptr(), max(t0.stride(0), t0.shape[1]),
                               t0.shape[1], layout, ids.data_ptr() if ids.shape[0] else None, ids.shape[0], factor)
    return arr, keep


def n_terms(arr, n):
    """kge_row_penalty_terms: host arithmetic."""
    return int(load_library().kge_row_penalty_terms(ctypes.byref(arr), n))


def row_offsets(arr, n):
    """The float offsets of the n blocks of the rows buffer and its length: n + 1 numbers (kge_row_penalty_row_offset)."""
    lib = load_library()
    return [int(lib.kge_row_penalty_row_offset(ctypes.byref(arr), n, s)) for s in range(n + 1)]


def row_penalty(streams, p, acc=None):
    """kge_row_penalty on the current stream: ``(loss, terms)`` -- the penalty of ``streams`` (tuples ``(layout, t0, t1,
    ids, factor)``) as a float32 device scalar, and its M per-occurrence terms.  ``acc``: a float32 device scalar the loss
    is also added to."""
    lib = load_library()
    _hip.require_cuda(*[x for s in streams for x in s[1:4]])
    arr, keep = descriptors(streams)
    n = len(streams)
    M = n_terms(arr, n)
    if M < 0:
        raise RuntimeError('torchkge_amd: kge_row_penalty takes at most %d streams, got %d' % (MAX_STREAMS, n))
    dev = streams[0][1].device if n else torch.device('cuda', torch.cuda.current_device())
    terms = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    nb = int(lib.kge_row_penalty_ws_bytes(M))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    with _on(dev):
        _check(lib.kge_row_penalty(ctypes.byref(arr), n, p, _p(terms), _p(loss), _p(acc), _p(ws), ws.numel(), _stream()),
               'kge_row_penalty')
    return loss, terms[:M]


def row_penalty_bwd(streams, p, go):
    """kge_row_penalty_bwd on the current stream: ``(rows, offsets)`` -- the rows buffer of the header's layout as one
    float32 vector and the float offsets of the streams' blocks in it (one more than streams: its length last).  ``go``:
    the incoming gradient, a float32 device scalar."""
    lib = load_library()
    arr, keep = descriptors(streams)
    n = len(streams)
    offs = row_offsets(arr, n)
    dev = go.device
    rows = torch.empty(max(offs[-1], 1), dtype=torch.float32, device=dev)
    with _on(dev):
        _check(lib.kge_row_penalty_bwd(ctypes.byref(arr), n, p, _p(go), _p(rows), _stream()), 'kge_row_penalty_bwd')
    return rows, offs


def row_penalty_grads(spec, p, ids, tables, go, needs, dense, row_grads=False, det=None):
    """The gradients of ``tables`` (None where ``needs`` is False) of ``go`` times the penalty of the streams ``spec``:
    tuples ``(layout, i0, i1, k, factor)`` naming tables[i0] (SPLIT: and tables[i1]) and ids[k].  Dense tables through
    _hip_det.reduce_rows -- one sort per distinct id vector, its order reused across the blocks -- or, with ``row_grads``,
    uncoalesced sparse gradients whose values are the blocks of the rows buffer; a table whose position is in ``dense``
    gets a dense gradient either way."""
    from ._hip_rows import sparse_rows
    streams = [(layout, tables[i0], None if i1 is None else tables[i1], ids[k], f) for layout, i0, i1, k, f in spec]
    rows, offs = row_penalty_bwd(streams, p, go)
    blocks = {}     # table position -> [(float offset, n, k)]
    for q, (layout, i0, i1, k, f) in enumerate(spec):
        n, d = ids[k].shape[0], tables[i0].shape[1]
        blocks.setdefault(i0, []).append((offs[q], n, k))
        if i1 is not None:
            blocks.setdefault(i1, []).append((offs[q] + n * d, n, k))
    grads = [None] * len(tables)
    perms = {}
    with _on(go.device):
        for ti, blks in blocks.items():
            if not needs[ti]:
                continue
            d = tables[ti].shape[1]
            if row_grads and ti not in dense:
                vals = [rows[o:o + n * d].view(n, d) for o, n, k in blks if n]
                keys = [ids[k] for o, n, k in blks if n]
                if len(vals) == 1:
                    grads[ti] = sparse_rows(keys[0], vals[0], tables[ti].shape)
                elif vals:
                    grads[ti] = sparse_rows(torch.cat(keys), torch.cat(vals), tables[ti].shape)
                continue
            g = grads[ti] = torch.zeros_like(tables[ti], memory_format=torch.contiguous_format)
            for o, n, k in blks:
                if n:
                    perms[k] = _hip_det.reduce_rows(rows.data_ptr() + 4 * o, d, d, ids[k], None, g, perm=perms.get(k), det=det)
    return grads


class RowPenalty(torch.autograd.Function):
    """loss = RowPenalty.apply(p, spec, dense, acc, n_ids, *ids, *tables): the penalty of the streams ``spec`` (tuples
    ``(layout, i0, i1, k, factor)`` into the ``n_ids`` id vectors and the tables behind them), differentiable with respect
    to the tables.  ``dense``: the positions of the tables whose gradient stays dense inside ``row_gradients()``."""

    @staticmethod
    def forward(ctx, p, spec, dense, acc, n_ids, *tensors):
        from .rowgrad import is_row_gradients
        ids = [i64c(x) for x in tensors[:n_ids]]
        tabs = [x.detach() for x in tensors[n_ids:]]
        ctx.p, ctx.spec, ctx.dense, ctx.n_ids = p, spec, dense, n_ids
        ctx.row_grads = is_row_gradients()      # read here: a loss built inside row_gradients() keeps the mode
        ctx.det = _hip_det.is_deterministic()   # ... and inside deterministic() the ordered reduction
        streams = [(layout, tabs[i0], None if i1 is None else tabs[i1], ids[k], f) for layout, i0, i1, k, f in spec]
        loss, _ = row_penalty(streams, p, acc)
        ctx.save_for_backward(*ids, *tabs)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        ids, tabs = list(ctx.saved_tensors[:ctx.n_ids]), list(ctx.saved_tensors[ctx.n_ids:])
        go = go.to(torch.float32).contiguous()
        grads = row_penalty_grads(ctx.spec, ctx.p, ids, tabs, go, ctx.needs_input_grad[5 + ctx.n_ids:], ctx.dense,
                                  row_grads=ctx.row_grads, det=ctx.det)
        return (None,) * (5 + ctx.n_ids) + tuple(grads)
