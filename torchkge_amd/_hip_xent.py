# -*- coding: utf-8 -*-
"""ctypes binding of the 1-vs-all criterion of libkge_hip.so (include/kge_hip_xent.h): ``xent_fwd`` / ``xent_bwd`` -- one
kge_lp_xent_fwd / kge_lp_xent_bwd on the current stream over a KGE_LP_DOT problem (``_hip.LpProblem``) -- and the geometry
the header publishes.  The (B, N) score matrix is never written: the workspace holds per-(row, candidate-chunk) partials.

The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature table of
their own because include/kge_hip.h and its ABI version do not change for them.  Nothing here synchronises or reads
back."""
import ctypes

import torch

from . import _hip, _hip_tile64
from ._hip import _vp, _i64, _check, _on, _stream, _p
from ._hip_tile64 import _size, _f32, BM, BN, MIN_TILES_PER_CHUNK, MAX_CHUNKS, MAX_K, KSLICE     # noqa: F401 (KGE_XENT_*)

_SIGNATURES = {
    'kge_lp_xent_fwd': [_vp, _vp, _f32, _vp, _vp, _vp, _size, _vp],
    'kge_lp_xent_bwd': [_vp, _vp, _f32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _size, _vp],
}
_WS_SIZES = ('kge_lp_xent_ws_bytes',)       # size_t f(int64_t B, int64_t N, int K0, int K1)
_WS_BYTES = {}      # (B, N, K0, K1) -> workspace bytes


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip_tile64.load_library(_SIGNATURES, _WS_SIZES, 'kge_lp_xent_chunks')


def ws_bytes(B, N, K0, K1=0):
    """kge_lp_xent_ws_bytes: host arithmetic, cached per shape."""
    return _hip_tile64.ws_bytes(_WS_BYTES, load_library, 'kge_lp_xent_ws_bytes', B, N, K0, K1)


def chunks(N):
    """kge_lp_xent_chunks: candidate chunks of an N-candidate problem (a function of N alone, capped at MAX_CHUNKS)."""
    return int(load_library().kge_lp_xent_chunks(N))


def _target(prob, target):
    _hip.require_cuda(target)
    target = _hip.i64c(target)
    if target.dim() != 1 or target.shape[0] != prob.B or target.device != prob.device:
        raise RuntimeError('torchkge_amd: the 1-vs-all criterion needs one target per query row on the queries\' device '
                           '(%d rows on %s, targets %s on %s)' % (prob.B, prob.device, tuple(target.shape), target.device))
    return target


def xent_fwd(prob, target, label_smoothing=0.0):
    """kge_lp_xent_fwd: ``(lse, row_loss)``, two float32 vectors of prob.B.  ``prob``: a KGE_LP_DOT ``_hip.LpProblem`` with
    c_base 0; ``target``: int64 in [0, N) per row (a precondition: nothing checks it on the device)."""
    lib = load_library()
    target = _target(prob, target)
    lse = torch.empty(prob.B, dtype=torch.float32, device=prob.device)
    row_loss = torch.empty(prob.B, dtype=torch.float32, device=prob.device)
    ws = _hip_tile64.workspace(prob, ws_bytes)
    with _on(prob.device):
        _check(lib.kge_lp_xent_fwd(ctypes.byref(prob.desc), _p(target), label_smoothing, _p(lse), _p(row_loss), _p(ws),
                                   ws.numel(), _stream()), 'kge_lp_xent_fwd')
    return lse, row_loss


def xent_bwd(prob, target, label_smoothing, lse, g, want_queries=True, want_tables=True):
    """kge_lp_xent_bwd: ``(dA, dT)`` -- lists of one gradient per segment (queries: (B, K), tables: (N, K)), or None for
    a group that is not wanted: its kernels are not launched.  ``g``: the float32 weight of every row's loss."""
    lib = load_library()
    target = _target(prob, target)
    dA, dT, launch = _hip_tile64.grad_groups(prob, want_queries, want_tables)
    if launch:
        ws = _hip_tile64.workspace(prob, ws_bytes)
        with _on(prob.device):
            _check(lib.kge_lp_xent_bwd(ctypes.byref(prob.desc), _p(target), label_smoothing, _p(lse), _p(_hip.f32c(g)),
                                       *(_hip_tile64.group_args(dA, dT) + [_p(ws), ws.numel(), _stream()])), 'kge_lp_xent_bwd')
    return dA, dT
