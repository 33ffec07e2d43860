# -*- coding: utf-8 -*-
"""ctypes binding of the fused training criterion of libkge_hip.so (include/kge_hip_train.h): ``pair_loss`` -- one
kge_pair_loss on the current stream -- and the ``torch.autograd.Function`` around it (``PairLoss``): the forward computes
the loss together with both gradient vectors, the backward scales them by the incoming scalar in one elementwise launch.

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
    'kge_pair_loss': [_int, _f32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _size, _vp],
}
_WS_SIZES = ('kge_pair_loss_ws_bytes',)         # size_t f(int64_t n)
_WS_BYTES = {}      # n -> workspace bytes
LOSS_MARGIN, LOSS_LOGISTIC, LOSS_BCE = 0, 1, 2  # KGE_LOSS_* of the header
CHUNK = 1024        # KGE_PAIR_LOSS_CHUNK: pairs per block and turn of the first stage


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    lib = _hip.bind(_SIGNATURES, _WS_SIZES, (_i64,), _size)
    lib.kge_pair_loss_max_blocks.argtypes, lib.kge_pair_loss_max_blocks.restype = [], _int
    return lib


def ws_bytes(n):
    """kge_pair_loss_ws_bytes: host arithmetic, cached per n."""
    nb = _WS_BYTES.get(n)
    if nb is None:
        nb = _WS_BYTES[n] = int(load_library().kge_pair_loss_ws_bytes(n))
    return nb


def max_blocks():
    """kge_pair_loss_max_blocks: the grid cap of the first stage."""
    return int(load_library().kge_pair_loss_max_blocks())


def _scores(x, name):
    if not x.is_cuda:
        _hip.require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 1:
        raise RuntimeError('torchkge_amd: pair_loss expects float32 vectors, got %s of %d dimensions for the %s scores'
                           % (x.dtype, x.dim(), name))
    return x if x.shape[0] < 2 or x.stride(0) == 1 else x.contiguous()


def pair_loss(kind, margin, pos, neg, acc=None, need_grad=True):
    """kge_pair_loss on the current stream: ``(loss, grads)`` -- the summed loss of the n pairs as a 0-d float32 tensor
    and, with ``need_grad``, one (2 n) vector holding d loss / d pos in its first half and d loss / d neg in its second
    (None otherwise: the value only).  ``pos`` / ``neg``: float32 CUDA vectors of one length, used where they lie (the
    two halves of one score vector are fine).  ``acc``: a float32 device scalar the loss is added to, or None."""
    lib = load_library()
    pos, neg = _scores(pos, 'positive'), _scores(neg, 'negative')
    n, dev = pos.shape[0], pos.device
    if neg.shape[0] != n or neg.device != dev:
        raise RuntimeError('torchkge_amd: pair_loss needs as many negative as positive scores on one device (%d on %s, '
                           '%d on %s)' % (n, dev, neg.shape[0], neg.device))
    loss = torch.empty((), dtype=torch.float32, device=dev)
    grads = torch.empty(2 * n, dtype=torch.float32, device=dev) if need_grad else None
    ws = torch.empty(max(ws_bytes(n), 8), dtype=torch.uint8, device=dev)
    gp = grads.data_ptr() if need_grad else None
    with _on(dev):
        _check(lib.kge_pair_loss(kind, margin, pos.data_ptr(), neg.data_ptr(), n, loss.data_ptr(),
                                 None if acc is None else acc.data_ptr(), gp, gp + 4 * n if need_grad else None,
                                 ws.data_ptr(), ws.numel(), _stream()), 'kge_pair_loss')
    return loss, grads


class PairLoss(torch.autograd.Function):
    """loss = PairLoss.apply(kind, margin, pos, neg, acc): differentiable with respect to both score vectors."""

    @staticmethod
    def forward(ctx, kind, margin, pos, neg, acc=None):
        need = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        loss, grads = pair_loss(kind, margin, pos.detach(), neg.detach(), acc, need_grad=need)
        ctx.n = pos.shape[0]
        if need:
            ctx.save_for_backward(grads)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        g = ctx.saved_tensors[0] * grad_out         # one launch for both halves, whatever the scalar
        return None, None, g[:ctx.n], g[ctx.n:], None
