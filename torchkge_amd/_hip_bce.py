# -*- coding: utf-8 -*-
"""ctypes binding of the K-vs-all criterion of libkge_hip.so (include/kge_hip_bce.h): ``bce_fwd`` / ``bce_bwd`` -- one
kge_lp_bce_fwd / kge_lp_bce_bwd on the current stream over a KGE_LP_DOT problem (``_hip.LpProblem``) and a CSR of true
candidates -- and the geometry the header publishes.  Neither the (B, N) score matrix nor a (B, N) label matrix is ever
written: the workspace holds per-(row, candidate-chunk) partials.

The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature table of
their own because include/kge_hip.h and its ABI version do not change for them.  Nothing here synchronises or reads
back."""
import ctypes

import torch

from . import _hip, _hip_tile64
from ._hip import _vp, _i64, _check, _on, _stream, _p
from ._hip_tile64 import _size, _f32, BM, BN, MIN_TILES_PER_CHUNK, MAX_CHUNKS, MAX_K, KSLICE     # noqa: F401 (KGE_BCE_*)

_SIGNATURES = {
    'kge_lp_bce_fwd': [_vp, _vp, _vp, _vp, _f32, _vp, _vp, _size, _vp],
    'kge_lp_bce_bwd': [_vp, _vp, _vp, _vp, _f32, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _size, _vp],
}
_WS_SIZES = ('kge_lp_bce_ws_bytes',)        # size_t f(int64_t B, int64_t N, int K0, int K1)
_WS_BYTES = {}      # (B, N, K0, K1) -> workspace bytes


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip_tile64.load_library(_SIGNATURES, _WS_SIZES, 'kge_lp_bce_chunks')


def ws_bytes(B, N, K0, K1=0):
    """kge_lp_bce_ws_bytes: host arithmetic, cached per shape."""
    return _hip_tile64.ws_bytes(_WS_BYTES, load_library, 'kge_lp_bce_ws_bytes', B, N, K0, K1)


def chunks(N):
    """kge_lp_bce_chunks: candidate chunks of an N-candidate problem (a function of N alone, capped at MAX_CHUNKS)."""
    return int(load_library().kge_lp_bce_chunks(N))


def _labels(prob, labels):
    """(seg_lo, seg_hi, targets) as the entries take them: two int64 vectors of prob.B, one int32 vector."""
    if not isinstance(labels, (tuple, list)) or len(labels) != 3:
        raise ValueError('torchkge_amd: the K-vs-all labels are (seg_lo, seg_hi, targets), as FilterIndex.lookup and '
                         'FilterIndex.targets give them')
    seg_lo, seg_hi, targets = labels
    _hip.require_cuda(seg_lo, seg_hi, targets)
    seg_lo, seg_hi = _hip.i64c(seg_lo), _hip.i64c(seg_hi)
    if targets.dtype != torch.int32 or targets.dim() != 1:
        raise RuntimeError('torchkge_amd: the K-vs-all label list is a one-dimensional int32 vector (FilterIndex.targets), '
                           'got %s of %d dimensions' % (targets.dtype, targets.dim()))
    for x in (seg_lo, seg_hi):
        if x.dim() != 1 or x.shape[0] != prob.B:
            raise RuntimeError('torchkge_amd: the K-vs-all criterion needs one label segment per query row (%d rows, '
                               'segment vectors of %s)' % (prob.B, tuple(x.shape)))
    if any(x.device != prob.device for x in (seg_lo, seg_hi, targets)):
        raise RuntimeError('torchkge_amd: the K-vs-all labels must live on the queries\' device (%s)' % (prob.device,))
    return seg_lo, seg_hi, targets.contiguous()


def bce_fwd(prob, labels, label_smoothing=0.0):
    """kge_lp_bce_fwd: ``row_loss``, a float32 vector of prob.B -- the sum over ALL candidates of the binary cross-entropy
    with logits.  ``prob``: a KGE_LP_DOT ``_hip.LpProblem`` with c_base 0; ``labels``: (seg_lo, seg_hi, targets), every
    segment strictly ascending in [0, N) (a precondition: nothing checks it on the device)."""
    lib = load_library()
    seg_lo, seg_hi, targets = _labels(prob, labels)
    row_loss = torch.empty(prob.B, dtype=torch.float32, device=prob.device)
    ws = _hip_tile64.workspace(prob, ws_bytes)
    with _on(prob.device):
        _check(lib.kge_lp_bce_fwd(ctypes.byref(prob.desc), _p(seg_lo), _p(seg_hi), _p(targets), label_smoothing,
                                  _p(row_loss), _p(ws), ws.numel(), _stream()), 'kge_lp_bce_fwd')
    return row_loss


def bce_bwd(prob, labels, label_smoothing, g, want_queries=True, want_tables=True):
    """kge_lp_bce_bwd: ``(dA, dT)`` -- lists of one gradient per segment (queries: (B, K), tables: (N, K)), or None for
    a group that is not wanted: its kernels are not launched.  ``g``: the float32 weight of every row's loss."""
    lib = load_library()
    seg_lo, seg_hi, targets = _labels(prob, labels)
    dA, dT, launch = _hip_tile64.grad_groups(prob, want_queries, want_tables)
    if launch:
        ws = _hip_tile64.workspace(prob, ws_bytes)
        with _on(prob.device):
            _check(lib.kge_lp_bce_bwd(ctypes.byref(prob.desc), _p(seg_lo), _p(seg_hi), _p(targets), label_smoothing,
                                      _p(_hip.f32c(g)), *(_hip_tile64.group_args(dA, dT) + [_p(ws), ws.numel(), _stream()])),
                   'kge_lp_bce_bwd')
    return dA, dT
