# -*- coding: utf-8 -*-
"""Criteria for training with K negatives per fact, on one fused HIP entry (kge_group_loss, include/kge_hip_group.h):

  * ``SelfAdversarialLoss`` -- self-adversarial negative sampling (Sun et al. 2019): per fact
    ``softplus(-(margin + p)) + sum_k w_k softplus(margin + n_k)`` with ``w = softmax(temperature * n)`` over the fact's
    own negatives, the weights constants of the gradient; ``temperature = 0`` is the uniform average;
  * ``SampledSoftmaxLoss`` -- the cross-entropy of the fact among itself and its negatives, ``logsumexp(p, n_1 .. n_K) - p``.

    criterion = SelfAdversarialLoss(margin=6.0, temperature=1.0, n_neg=64)
    loss = criterion(*model(h, t, r, nh, nt))       # nh, nt of 64 * B entries in tile order (sampler.corrupt_batch)
    loss.backward()

The scores are those ``Model.forward`` returns: the negatives in tile order -- negative k of fact i at ``k * B + i``, the
order of ``heads.repeat(n_neg)`` -- and the positives either B long or repeated to ``B * n_neg`` (the first B are used).
Loss and both gradients come out of one call; nothing is read back, and the outputs stay finite where the written-out
softmax / logsigmoid saturate.  There is no CPU path."""
from torch.nn import Module

from .. import _hip, _hip_group


class _GroupCriterion(Module):
    kind = None
    margin = 0.0
    temperature = 0.0

    def __init__(self, n_neg=None, reduction='sum'):
        super().__init__()
        if reduction not in ('sum', 'mean'):
            raise ValueError("reduction is 'sum' or 'mean', got %r" % (reduction,))
        if n_neg is not None and int(n_neg) < 1:
            raise ValueError('n_neg must be at least 1, got %r' % (n_neg,))
        self.n_neg = None if n_neg is None else int(n_neg)
        self.reduction = reduction

    def forward(self, positive_triplets, negative_triplets, acc=None, weights=None):
        """The loss summed (or averaged) over the facts.  ``acc``: a float32 device scalar the returned loss is also
        added to (a running epoch sum).  ``weights``: one float32 weight per fact (subsampling weights), or None."""
        B = _hip_group.split(positive_triplets.shape[0], negative_triplets.numel(), self.n_neg)
        _hip.require_cuda(positive_triplets, negative_triplets, weights)
        pos = positive_triplets[:B]             # the repeated form: repeat's backward hands the gradient on once
        if self.reduction == 'sum' or B == 0:
            return _hip_group.GroupLoss.apply(self.kind, self.margin, self.temperature, pos, negative_triplets,
                                              self.n_neg, weights, acc)
        loss = _hip_group.GroupLoss.apply(self.kind, self.margin, self.temperature, pos, negative_triplets, self.n_neg,
                                          weights, None) / B
        if acc is not None:
            acc.add_(loss.detach())
        return loss


class SelfAdversarialLoss(_GroupCriterion):
    """sum_i softplus(-(margin + f(pos_i))) + sum_k softmax_k(temperature * f(neg_ik)) * softplus(margin + f(neg_ik))."""
    kind = _hip_group.GROUP_NSSA

    def __init__(self, margin, temperature=1.0, n_neg=None, reduction='sum'):
        super().__init__(n_neg, reduction)
        if not 0.0 <= float(temperature) < float('inf'):
            raise ValueError('temperature must be finite and not negative, got %r' % (temperature,))
        self.margin = float(margin)
        self.temperature = float(temperature)


class SampledSoftmaxLoss(_GroupCriterion):
    """sum_i logsumexp(f(pos_i), f(neg_i1), ..., f(neg_iK)) - f(pos_i)."""
    kind = _hip_group.GROUP_SOFTMAX

    def __init__(self, n_neg=None, reduction='sum'):
        super().__init__(n_neg, reduction)
