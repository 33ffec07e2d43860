# -*- coding: utf-8 -*-
"""ctypes binding of the grouped training criteria of libkge_hip.so (include/kge_hip_group.h): ``group_loss`` -- one
kge_group_loss on the current stream -- and the ``torch.autograd.Function`` around it (``GroupLoss``): the forward
computes the loss together with both gradients, the backward scales them by the incoming scalar in one elementwise launch.

The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature table of
their own because include/kge_hip.h and its ABI version do not change for them.  Nothing here synchronises or reads
back."""
import ctypes

import torch

from . import _hip
from ._hip import _vp, _i64, _int, _check, _on, _stream

_size = ctypes.c_size_t
_f32 = ctypes.c_float
_SIGNATURES = {
    'kge_group_loss': [_int, _f32, _f32, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _size, _vp],
}
_WS_SIZES = ('kge_group_loss_ws_bytes',)        # size_t f(int64_t B, int64_t K)
_WS_BYTES = {}      # (B, K) -> workspace bytes
GROUP_NSSA, GROUP_SOFTMAX = 0, 1                # KGE_GROUP_* of the header
ROWS, SLICES, MIN_K_PER_CHUNK, MAX_CHUNKS = 256, 4, 32, 16      # the header's geometry


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    lib = _hip.bind(_SIGNATURES, _WS_SIZES, (_i64, _i64), _size)
    lib.kge_group_loss_chunks.argtypes, lib.kge_group_loss_chunks.restype = [_i64], _int
    return lib


def ws_bytes(B, K):
    """kge_group_loss_ws_bytes: host arithmetic, cached per shape."""
    nb = _WS_BYTES.get((B, K))
    if nb is None:
        nb = _WS_BYTES[(B, K)] = int(load_library().kge_group_loss_ws_bytes(B, K))
    return nb


def chunks(K):
    """kge_group_loss_chunks: the chunk blocks K negatives are cut into."""
    return int(load_library().kge_group_loss_chunks(K))


def _vector(x, name):
    if not x.is_cuda:
        _hip.require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 1:
        raise RuntimeError('torchkge_amd: group_loss expects a float32 vector, got %s of %d dimensions for the %s'
                           % (x.dtype, x.dim(), name))
    return x if x.shape[0] < 2 or x.stride(0) == 1 else x.contiguous()


def split(n_pos, n_negs, n_neg):
    """B of ``n_negs`` negative scores in groups of ``n_neg``; ``n_pos`` must be B or B * n_neg."""
    if n_neg is None:
        raise ValueError('torchkge_amd: a grouped criterion needs n_neg (negatives per fact): pass it, or let the '
                         'Trainer set it')
    if n_neg < 1 or n_negs % n_neg != 0:
        raise ValueError('torchkge_amd: %d negative scores are not %d per fact' % (n_negs, n_neg))
    B = n_negs // n_neg
    if n_pos not in (B, B * n_neg):
        raise ValueError('torchkge_amd: %d positive scores for %d facts of %d negatives each (expected %d, or %d as '
                         'Model.forward repeats them)' % (n_pos, B, n_neg, B, B * n_neg))
    return B


def group_loss(kind, margin, temperature, pos, neg, n_neg, weights=None, acc=None, need_grad=True):
    """kge_group_loss on the current stream: ``(loss, row_loss, grads)`` -- the summed loss of the B facts as a 0-d
    float32 tensor, the B row terms, and with ``need_grad`` one (B + n_neg * B) vector holding d loss / d pos in its first B
    entries and d loss / d neg behind them, laid out like ``neg`` (None otherwise: the value only).

    ``pos``: B float32 CUDA scores, or B * n_neg of which the first B count (``pos.repeat(n_neg)``).  ``neg``: a
    flat vector of n_neg * B scores in tile order (negative k of fact i at k * B + i), or an (n_neg, B) matrix with
    unit column stride whose rows may be padded; both are used where they lie.  ``weights``: B float32 row weights or
    None.  ``acc``: a float32 device scalar the loss is added to, or None."""
    lib = load_library()
    _hip.require_cuda(pos, neg, weights)
    if neg.dim() == 2:
        if neg.dtype != torch.float32:
            raise RuntimeError('torchkge_amd: group_loss expects float32 scores, got %s' % neg.dtype)
        if neg.shape[0] != n_neg:
            raise ValueError('torchkge_amd: a negative score matrix of %d rows for n_neg = %d' % (neg.shape[0], n_neg))
        if (neg.shape[1] > 1 and neg.stride(1) != 1) or (n_neg > 1 and neg.stride(0) < neg.shape[1]):
            neg = neg.contiguous()
        ld = neg.stride(0) if n_neg > 1 and neg.shape[1] > 0 else max(neg.shape[1], 1)
        n_negs = neg.shape[0] * neg.shape[1]
    else:
        neg = _vector(neg, 'negative scores')
        n_negs, ld = neg.shape[0], None
    pos = _vector(pos, 'positive scores')
    B = split(pos.shape[0], n_negs, n_neg)
    dev = pos.device
    if ld is None:
        ld = max(B, 1)
    if neg.device != dev:
        raise RuntimeError('torchkge_amd: group_loss needs both score vectors on one device (%s, %s)' % (dev, neg.device))
    if weights is not None:
        weights = _vector(weights, 'row weights')
        if weights.shape[0] != B or weights.device != dev:
            raise RuntimeError('torchkge_amd: group_loss needs one row weight per fact on the scores\' device (%d for %d '
                               'facts)' % (weights.shape[0], B))
    loss = torch.empty((), dtype=torch.float32, device=dev)
    row_loss = torch.empty(B, dtype=torch.float32, device=dev)
    grads = torch.empty(B + n_neg * B, dtype=torch.float32, device=dev) if need_grad else None
    ws = torch.empty(max(ws_bytes(B, n_neg), 16), dtype=torch.uint8, device=dev)
    gp = grads.data_ptr() if need_grad else None
    with _on(dev):
        _check(lib.kge_group_loss(kind, margin, temperature, pos.data_ptr(), neg.data_ptr(), ld,
                                  None if weights is None else weights.data_ptr(), B, n_neg, loss.data_ptr(),
                                  None if acc is None else acc.data_ptr(), row_loss.data_ptr(), gp,
                                  gp + 4 * B if need_grad else None, max(B, 1), ws.data_ptr(), ws.numel(), _stream()),
               'kge_group_loss')
    return loss, row_loss, grads


class GroupLoss(torch.autograd.Function):
    """loss = GroupLoss.apply(kind, margin, temperature, pos, neg, n_neg, weights, acc): differentiable with respect to
    both score vectors (``pos`` of B entries; the weights are constants)."""

    @staticmethod
    def forward(ctx, kind, margin, temperature, pos, neg, n_neg, weights=None, acc=None):
        need = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        loss, _, grads = group_loss(kind, margin, temperature, pos.detach(), neg.detach(), n_neg,
                                    None if weights is None else weights.detach(), acc, need_grad=need)
        ctx.n_pos, ctx.neg_shape = pos.shape[0], neg.shape
        if need:
            ctx.save_for_backward(grads)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        g = ctx.saved_tensors[0] * grad_out         # one launch for both gradients, whatever the scalar
        B = g.shape[0] - ctx.neg_shape.numel()
        gp = g[:B]
        if ctx.n_pos != B:                          # the repeated form: only the first B entries were read
            gp = torch.cat([gp, gp.new_zeros(ctx.n_pos - B)])
        return None, None, None, gp, g[B:].view(ctx.neg_shape), None, None, None
