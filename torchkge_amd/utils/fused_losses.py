# -*- coding: utf-8 -*-
"""The three training criteria of ``utils/losses.py`` on one fused HIP kernel (kge_pair_loss, include/kge_hip_train.h):
the loss and both gradient vectors come out of ONE launch pair, the backward is one elementwise multiply, and the
gradients are closed forms that stay finite where ``sigmoid`` / ``exp`` saturate in fp32 (a positive of score 30 under
``BinaryCrossEntropyLoss``, a score beyond 88 under ``LogisticLoss``: NaN gradients there).

    criterion = FusedMarginLoss(0.5)            # or fused_for(MarginLoss(0.5))
    loss = criterion(*model(h, t, r, nh, nt))   # CUDA float32 vectors of equal length
    loss.backward()

The classes of ``utils/losses.py`` are untouched; these sum in another order (a fixed fp64 tree) and so agree with them
to rounding, not bit for bit."""
from torch.nn import Module

from .. import _hip_train
from .losses import MarginLoss, LogisticLoss, BinaryCrossEntropyLoss


class _FusedPairCriterion(Module):
    kind = None
    margin = 0.0

    def forward(self, positive_triplets, negative_triplets, acc=None):
        """The summed loss.  ``acc``: a float32 device scalar the loss is also added to (a running epoch sum)."""
        return _hip_train.PairLoss.apply(self.kind, self.margin, positive_triplets, negative_triplets, acc)


class FusedMarginLoss(_FusedPairCriterion):
    """sum_i max(0, margin - f(pos_i) + f(neg_i)); a hinge of exactly zero passes the gradient, as clamp_min does."""
    kind = _hip_train.LOSS_MARGIN

    def __init__(self, margin):
        super().__init__()
        self.margin = float(margin)


class FusedLogisticLoss(_FusedPairCriterion):
    """sum_i softplus(-f(pos_i)) + softplus(f(neg_i))."""
    kind = _hip_train.LOSS_LOGISTIC


class FusedBinaryCrossEntropyLoss(_FusedPairCriterion):
    """The logistic terms, each cut off at 100 (BCELoss's logarithms at -100) with gradient 0 beyond."""
    kind = _hip_train.LOSS_BCE


def fused_for(criterion):
    """The fused counterpart of an instance of MarginLoss / LogisticLoss / BinaryCrossEntropyLoss, None for anything
    else (a subclass may have changed the terms: only the three classes themselves count)."""
    cls = type(criterion)
    if cls is MarginLoss:
        return FusedMarginLoss(criterion.margin)
    if cls is LogisticLoss:
        return FusedLogisticLoss()
    if cls is BinaryCrossEntropyLoss:
        return FusedBinaryCrossEntropyLoss()
    return None
