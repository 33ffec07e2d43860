# -*- coding: utf-8 -*-
"""Dissimilarities of the reference (utils/dissimilarities.py:11-54) on the HIP
kernels.  ``l2_dissimilarity`` is the SQUARED L2 norm.  All of them are
differentiable like the reference's torch expressions (user-defined models call
``model.dissimilarity`` inside their own scoring functions): the forward value
comes from the HIP kernel, the backward is the closed form
d/da ||a-b||_1 = sign(a-b), d/da ||a-b||_2^2 = 2 (a-b), and for the torus ones
the derivative of the branch each ``min`` took (zero at an exact tie, where
torch splits the gradient half and half between two opposite terms).

The torus dissimilarities are applied literally to x = a - b, with no
wrap-around, as the reference does: for |x| > 1 a term is negative."""
import math

import torch

from .. import _hip


def _rowwise(a, b, mode):
    a, b = torch.broadcast_tensors(a, b)
    shape = a.shape[:-1]
    K = a.shape[-1]
    q = a.reshape(-1, K)
    c = b.reshape(-1, 1, K)
    out = _hip.lp_scores_batched(mode, q, c)     # one candidate per row
    return (-out).reshape(shape)


def _branch(lo, hi):
    """+1 where the min took its first argument, -1 where the second, 0 at a tie."""
    return (lo < hi).to(lo.dtype) - (lo > hi).to(lo.dtype)


def _grad(diff, mode):
    """d diss / d a (elementwise, a - b = diff)."""
    if mode == _hip.LP_L1_DIRECT:
        return torch.sign(diff)
    if mode == _hip.LP_L2_DIRECT:
        return 2.0 * diff
    if mode == _hip.LP_TORUS_L1:        # 2 min(|x|, 1 - |x|)
        a = diff.abs()
        return 2.0 * _branch(a, 1.0 - a) * torch.sign(diff)
    if mode == _hip.LP_TORUS_L2:        # 4 min(x^2, 1 - x^2)
        v = diff * diff
        return 4.0 * _branch(v, 1.0 - v) * (2.0 * diff)
    u = torch.minimum(diff, 1.0 - diff)  # sum 2 (1 - cos(2 pi u)) / 4
    return _branch(diff, 1.0 - diff) * (math.pi * torch.sin(2.0 * math.pi * u))


class _Dissimilarity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, mode):
        ctx.mode = mode
        ctx.save_for_backward(a, b)
        return _rowwise(a.detach(), b.detach(), mode)

    @staticmethod
    def backward(ctx, grad_out):
        a, b = ctx.saved_tensors
        diff = a - b                                   # broadcast shape
        g = _grad(diff, ctx.mode) * grad_out.unsqueeze(-1)
        ga = g.sum_to_size(a.shape) if ctx.needs_input_grad[0] else None
        gb = (-g).sum_to_size(b.shape) if ctx.needs_input_grad[1] else None
        return ga, gb, None


def _diss(a, b, mode):
    assert len(a.shape) == len(b.shape)
    _hip.require_cuda(a, b)
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        return _Dissimilarity.apply(a, b, mode)
    return _rowwise(a, b, mode)


def l1_dissimilarity(a, b):
    """||a - b||_1 along the last dim (dissimilarities.py:11-16)."""
    return _diss(a, b, _hip.LP_L1_DIRECT)


def l2_dissimilarity(a, b):
    """||a - b||_2^2 along the last dim (dissimilarities.py:19-25)."""
    return _diss(a, b, _hip.LP_L2_DIRECT)


def l1_torus_dissimilarity(a, b):
    """2 sum min(|a - b|, 1 - |a - b|) along the last dim (dissimilarities.py:28-34)."""
    return _diss(a, b, _hip.LP_TORUS_L1)


def l2_torus_dissimilarity(a, b):
    """4 sum min((a - b)^2, 1 - (a - b)^2) along the last dim (dissimilarities.py:37-43)."""
    return _diss(a, b, _hip.LP_TORUS_L2)


def el2_torus_dissimilarity(a, b):
    """sum 2 (1 - cos(2 pi min(a - b, 1 - (a - b)))) / 4 along the last dim (dissimilarities.py:46-54)."""
    return _diss(a, b, _hip.LP_TORUS_EL2)
