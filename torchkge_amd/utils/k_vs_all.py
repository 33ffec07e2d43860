# -*- coding: utf-8 -*-
"""K-vs-all training: the binary cross-entropy with logits of every query row over ALL candidates against the set of its
known true answers, on the engine's own scores and without the (B, N) score matrix, a (B, N) label matrix or the (B, N)
gradient (kge_lp_bce_fwd / kge_lp_bce_bwd, include/kge_hip_bce.h).

    loss = all_candidates_bce(Q, E, (seg_lo, seg_hi, targets))      # F.binary_cross_entropy_with_logits(Q @ E.T, Y)
    loss = all_candidates_bce((Q0, Q1), (E_re, E_im), labels)       # two segments: s = Q0 . E_re + Q1 . E_im
    loss = model.k_vs_all_loss(h, r, labels, side='tail')           # DistMultModel / ComplExModel

A query is a key -- (h, r) on the tail side, (t, r) on the head side -- and its label is a segment of a sorted CSR:
``labels = (seg_lo, seg_hi, targets)`` are what ``FilterIndex.lookup`` returns and the index's ``targets``, used in
place; row i's true set is ``targets[seg_lo[i]:seg_hi[i]]``.

Label smoothing mixes every label with the uniform distribution over the N candidates, the convention of
one_vs_all: y = (1 - eps) * [c in set] + eps / N.

The scores are those of ``_hip.LpProblem(LP_DOT, ...)``: the bits ``scores()`` / ``pair_scores()`` give and the evaluator
ranks.  There is no fallback: tensors that are not on the GPU raise."""
import torch

from .. import _hip, _hip_bce
from . import all_candidates
from .all_candidates import REDUCTIONS      # noqa: F401
from .one_vs_all import _QueryRows

SIDES = ('tail', 'head')


class _AllCandidatesBce(torch.autograd.Function):
    """row_loss = _AllCandidatesBce.apply(seg_lo, seg_hi, targets, label_smoothing, n_seg, *queries, *tables):
    differentiable in the queries and the tables.  The backward recomputes the scores tile by tile and needs nothing the
    forward wrote; ``needs_input_grad`` decides which of the two backward products are launched."""

    @staticmethod
    def forward(ctx, seg_lo, seg_hi, targets, label_smoothing, n_seg, *ops):
        ops, prob = all_candidates.forward_problem(ctx, label_smoothing, n_seg, ops)
        row_loss = _hip_bce.bce_fwd(prob, (seg_lo, seg_hi, targets), label_smoothing)
        ctx.save_for_backward(seg_lo, seg_hi, targets, *ops)
        return row_loss

    @staticmethod
    def backward(ctx, grad_rows):
        def bwd(prob, labels, g, **want):
            return _hip_bce.bce_bwd(prob, labels, ctx.eps, g, **want)
        return all_candidates.backward(ctx, grad_rows, 5, 3, bwd)


def all_candidates_bce(queries, tables, labels, label_smoothing=0.0, reduction='mean'):
    """``F.binary_cross_entropy_with_logits(S, Y, reduction=...)`` of S[i, c] = queries[i] . tables[c] and
    Y[i, c] = (1 - eps) * [c in targets[seg_lo[i]:seg_hi[i]]] + eps / N, without S and without Y.

    ``queries``: a (B, K) float32 matrix on the GPU, or a pair (B, K0), (B, K1); ``tables``: (N, K) or the matching pair
    (N, K0), (N, K1) -- the score is the sum over the segments, K0 + K1 <= 1024.  ``labels``: (seg_lo, seg_hi, targets)
    -- int64 (B), int64 (B), int32; every segment strictly ascending with values in [0, N) (a precondition; nothing
    checks it on the device -- a FilterIndex built with n_values = N satisfies it).  ``reduction``: 'none' gives the B row
    sums over the candidates, 'sum' their sum, 'mean' the sum divided by B * N (torch's definition).  Differentiable in
    the queries and the tables; the table gradient is dense, (N, K).  Deterministic whatever
    ``torchkge_amd.determinism`` says: no float atomic, a fixed order."""
    all_candidates.check_options('all_candidates_bce', label_smoothing, reduction)
    if not isinstance(labels, (tuple, list)) or len(labels) != 3:
        raise ValueError('all_candidates_bce: labels are (seg_lo, seg_hi, targets), got %r' % (type(labels).__name__,))
    qs, ts = all_candidates.check_operands('all_candidates_bce', queries, tables, labels)
    B, N = qs[0].shape[0], ts[0].shape[0]
    seg_lo, seg_hi, targets = labels
    if seg_lo.dim() != 1 or seg_hi.dim() != 1 or seg_lo.shape[0] != B or seg_hi.shape[0] != B:
        raise ValueError('all_candidates_bce: one label segment per query row: %d rows, seg_lo %s, seg_hi %s'
                         % (B, tuple(seg_lo.shape), tuple(seg_hi.shape)))
    rows = _AllCandidatesBce.apply(seg_lo, seg_hi, targets, float(label_smoothing), len(qs), *(qs + ts))
    if reduction == 'none':
        return rows
    total = rows.sum()
    return total if reduction == 'sum' else total / float(B * N)


def k_vs_all_loss(model, ent_idx, r_idx, labels, side, label_smoothing=0.0, reduction='mean'):
    """``Model.k_vs_all_loss`` of DistMultModel / ComplExModel (see there)."""
    if side not in SIDES:
        raise ValueError("k_vs_all_loss: side is 'tail' or 'head', got %r" % (side,))
    model._check_unsharded('k_vs_all_loss')
    tables = model._tables()
    _hip.require_cuda(ent_idx, r_idx, *tables)
    n_et = len(model._ENT_TABLES)
    # the key's entity is the head of a tail-side query and the tail of a head-side one; _QueryRows reads only that one
    q = _QueryRows.apply(model._hip_kind(), side, model._d_ent, model._d_rel, ent_idx, ent_idx, r_idx, *tables)
    q = q if isinstance(q, tuple) else (q,)
    return all_candidates_bce(q, tuple(tables[:n_et]), labels, label_smoothing, reduction)
