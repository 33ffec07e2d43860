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

from . import _hip
from ._hip import _vp, _i64, _int, _check, _on, _stream, _p

_size = ctypes.c_size_t
_f32 = ctypes.c_float
_SIGNATURES = {
    'kge_lp_bce_fwd': [_vp, _vp, _vp, _vp, _f32, _vp, _vp, _size, _vp],
    'kge_lp_bce_bwd': [_vp, _vp, _vp, _vp, _f32, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _size, _vp],
}
_WS_SIZES = ('kge_lp_bce_ws_bytes',)        # size_t f(int64_t B, int64_t N, int K0, int K1)
_WS_BYTES = {}      # (B, N, K0, K1) -> workspace bytes
# the constants of the header
BM, BN = 64, 64                 # KGE_BCE_BM, KGE_BCE_BN: queries per row panel, candidates per tile
MIN_TILES_PER_CHUNK = 4         # KGE_BCE_MIN_TILES_PER_CHUNK
MAX_CHUNKS = 32                 # KGE_BCE_MAX_CHUNKS
MAX_K = 1024                    # KGE_BCE_MAX_K
KSLICE = 512                    # KGE_BCE_KSLICE


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    lib = _hip.bind(_SIGNATURES, _WS_SIZES, (_i64, _i64, _int, _int), _size)
    lib.kge_lp_bce_chunks.argtypes, lib.kge_lp_bce_chunks.restype = [_i64], _int
    return lib


def ws_bytes(B, N, K0, K1=0):
    """kge_lp_bce_ws_bytes: host arithmetic, cached per shape."""
    key = (B, N, K0, K1)
    nb = _WS_BYTES.get(key)
    if nb is None:
        nb = _WS_BYTES[key] = int(load_library().kge_lp_bce_ws_bytes(B, N, K0, K1))
    return nb


def chunks(N):
    """kge_lp_bce_chunks: candidate chunks of an N-candidate problem (a function of N alone, capped at MAX_CHUNKS)."""
    return int(load_library().kge_lp_bce_chunks(N))


def _workspace(prob):
    d = prob.desc
    return torch.empty(max(ws_bytes(int(d.B), int(d.N), int(d.K0), int(d.K1)), 16), dtype=torch.uint8, device=prob.device)


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
    ws = _workspace(prob)
    with _on(prob.device):
        _check(lib.kge_lp_bce_fwd(ctypes.byref(prob.desc), _p(seg_lo), _p(seg_hi), _p(targets), label_smoothing,
                                  _p(row_loss), _p(ws), ws.numel(), _stream()), 'kge_lp_bce_fwd')
    return row_loss


def bce_bwd(prob, labels, label_smoothing, g, want_queries=True, want_tables=True):
    """kge_lp_bce_bwd: ``(dA, dT)`` -- lists of one gradient per segment (queries: (B, K), tables: (N, K)), or None for
    a group that is not wanted: its kernels are not launched.  ``g``: the float32 weight of every row's loss."""
    lib = load_library()
    seg_lo, seg_hi, targets = _labels(prob, labels)
    d, dev = prob.desc, prob.device
    segs = [int(d.K0)] + ([int(d.K1)] if d.K1 else [])
    dA = [torch.empty(prob.B, k, dtype=torch.float32, device=dev) for k in segs] if want_queries else None
    dT = [torch.empty(prob.N, k, dtype=torch.float32, device=dev) for k in segs] if want_tables else None
    if not (want_queries or want_tables) or prob.B == 0:
        for grp in (dA, dT):
            for x in grp or ():
                x.zero_()
        return dA, dT
    ws = _workspace(prob)

    def args(grp):
        out = []
        for j in range(2):
            x = grp[j] if grp is not None and j < len(grp) else None
            out += [_p(x), 0 if x is None else x.stride(0)]
        return out

    with _on(dev):
        _check(lib.kge_lp_bce_bwd(ctypes.byref(d), _p(seg_lo), _p(seg_hi), _p(targets), label_smoothing, _p(_hip.f32c(g)),
                                  *(args(dA) + args(dT) + [_p(ws), ws.numel(), _stream()])), 'kge_lp_bce_bwd')
    return dA, dT
