# -*- coding: utf-8 -*-
"""1-vs-all training: the softmax cross-entropy of every query row over ALL candidates, on the engine's own scores and
without the (B, N) score matrix, its softmax or its gradient (kge_lp_xent_fwd / kge_lp_xent_bwd, include/kge_hip_xent.h).

    loss = all_candidates_cross_entropy(Q, E, t)                    # F.cross_entropy(Q @ E.T, t), never materialised
    loss = all_candidates_cross_entropy((Q0, Q1), (E_re, E_im), t)  # two segments: s = Q0 . E_re + Q1 . E_im
    loss = model.one_vs_all_loss(h, t, r)                           # DistMultModel / ComplExModel

The scores are those of ``_hip.LpProblem(LP_DOT, ...)``: the bits ``scores()`` / ``pair_scores()`` give and the evaluator
ranks.  There is no fallback: tensors that are not on the GPU raise."""
import torch

from .. import _hip, _hip_det, _hip_xent
from . import all_candidates
from .all_candidates import REDUCTIONS      # noqa: F401

SIDES = ('both', 'tail', 'head')


class _AllCandidatesXent(torch.autograd.Function):
    """row_loss = _AllCandidatesXent.apply(target, label_smoothing, n_seg, *queries, *tables): differentiable in the
    queries and the tables.  ``lse`` is saved for the backward, which recomputes the scores tile by tile;
    ``needs_input_grad`` decides which of the two backward products are launched."""

    @staticmethod
    def forward(ctx, target, label_smoothing, n_seg, *ops):
        ops, prob = all_candidates.forward_problem(ctx, label_smoothing, n_seg, ops)
        lse, row_loss = _hip_xent.xent_fwd(prob, target, label_smoothing)
        ctx.save_for_backward(target, lse, *ops)
        return row_loss

    @staticmethod
    def backward(ctx, grad_rows):
        def bwd(prob, saved, g, **want):
            return _hip_xent.xent_bwd(prob, saved[0], ctx.eps, saved[1], g, **want)
        return all_candidates.backward(ctx, grad_rows, 3, 2, bwd)


def all_candidates_cross_entropy(queries, tables, target, label_smoothing=0.0, reduction='mean'):
    """``F.cross_entropy(S, target, label_smoothing=..., reduction=...)`` of S[i, c] = queries[i] . tables[c] without S.

    ``queries``: a (B, K) float32 matrix on the GPU, or a pair (B, K0), (B, K1); ``tables``: (N, K) or the matching pair
    (N, K0), (N, K1) -- the score is the sum over the segments, K0 + K1 <= 1024.  ``target``: int64 in [0, N) per row (a
    precondition; nothing checks it on the device).  Differentiable in the queries and the tables; the table gradient is
    dense, (N, K).  Deterministic whatever ``torchkge_amd.determinism`` says: no float atomic, a fixed order."""
    all_candidates.check_options('all_candidates_cross_entropy', label_smoothing, reduction)
    qs, ts = all_candidates.check_operands('all_candidates_cross_entropy', queries, tables, (target,))
    rows = _AllCandidatesXent.apply(target, float(label_smoothing), len(qs), *(qs + ts))
    if reduction == 'none':
        return rows
    return rows.sum() if reduction == 'sum' else rows.mean()


# ---------------------------------------------------------------------------
# DistMult / ComplEx: the query rows of kge_lp_prep, differentiable in the tables
# ---------------------------------------------------------------------------
def _complex_rows(a, b, er, ei, rr, ri, tail):
    """Gradient rows (d er, d ei, d rr, d ri) of ComplEx's query rows from (a, b) = (d Q0, d Q1).
    tail: Q0 = er rr - ei ri, Q1 = er ri + ei rr;  head: Q0 = rr er + ri ei, Q1 = rr ei - ri er."""
    if tail:
        return a * rr + b * ri, b * rr - a * ri, a * er + b * ei, b * er - a * ei
    return a * rr - b * ri, a * ri + b * rr, a * er + b * ei, a * ei - b * er


class _QueryRows(torch.autograd.Function):
    """The query rows of one side of a batch -- the forward IS ``_hip.lp_prep``, what the evaluator scores -- with a
    backward into the model's tables: elementwise products on the gathered rows, reduced into dense table gradients by
    ``_hip_det.reduce_rows`` (the ordered, atomic-free sum in deterministic mode)."""

    @staticmethod
    def forward(ctx, kind, side, d_ent, d_rel, h, t, r, *tables):
        tabs = [x.detach() for x in tables]
        cplx = kind == _hip.COMPLEX
        out = _hip.lp_prep(kind, _hip.side_code(side), tabs, d_ent, d_rel, h, t, r, want_q1=cplx)
        ctx.kind, ctx.side = kind, side
        ctx.save_for_backward(h, t, r, *tabs)
        if cplx:
            return out[0], out[1]
        return out[0]

    @staticmethod
    def backward(ctx, *gq):
        h, t, r = [_hip.i64c(x) for x in ctx.saved_tensors[:3]]
        tabs = ctx.saved_tensors[3:]
        needs = ctx.needs_input_grad[7:]
        cplx = ctx.kind == _hip.COMPLEX
        n_et = 2 if cplx else 1
        B = h.shape[0]
        parts = {'tail': [(h, True, 0)], 'head': [(t, False, 0)], 'both': [(h, True, 0), (t, False, B)]}[ctx.side]
        gq = [_hip.f32c(g) for g in gq]
        ent_rows = [[] for _ in range(n_et)]
        rel_rows = [[] for _ in range(n_et)]
        for idx, tail, off in parts:
            e = [_hip.gather_rows(_hip.f32c(x), idx) for x in tabs[:n_et]]
            rel = [_hip.gather_rows(_hip.f32c(x), r) for x in tabs[n_et:]]
            if cplx:
                rows = _complex_rows(gq[0][off:off + B], gq[1][off:off + B], e[0], e[1], rel[0], rel[1], tail)
                for j in range(2):
                    ent_rows[j].append(rows[j])
                    rel_rows[j].append(rows[2 + j])
            else:       # DistMult: q = e * r on either side
                ent_rows[0].append(gq[0][off:off + B] * rel[0])
                rel_rows[0].append(gq[0][off:off + B] * e[0])
        ent_ids = torch.cat([p[0] for p in parts]) if len(parts) > 1 else parts[0][0]
        rel_ids = torch.cat([r] * len(parts)) if len(parts) > 1 else r
        det = _hip_det.is_deterministic()
        grads = [None] * len(tabs)
        with _hip._on(h.device):
            for group, ids, first in ((ent_rows, ent_ids, 0), (rel_rows, rel_ids, n_et)):
                perm = None     # one sort per id set
                for j, rows in enumerate(group):
                    if not needs[first + j]:
                        continue
                    rows = torch.cat(rows) if len(rows) > 1 else rows[0].contiguous()
                    g = grads[first + j] = torch.zeros_like(tabs[first + j], memory_format=torch.contiguous_format)
                    if ids.shape[0]:
                        perm = _hip_det.reduce_rows(rows, rows.stride(0), g.shape[1], ids, None, g, perm=perm, det=det)
        return (None,) * 7 + tuple(grads)


def one_vs_all_loss(model, h_idx, t_idx, r_idx, side='both', label_smoothing=0.0, reduction='mean'):
    """``Model.one_vs_all_loss`` of DistMultModel / ComplExModel (see there)."""
    if side not in SIDES:
        raise ValueError("one_vs_all_loss: side is 'both', 'tail' or 'head', got %r" % (side,))
    model._check_unsharded('one_vs_all_loss')
    tables = model._tables()
    _hip.require_cuda(h_idx, t_idx, r_idx, *tables)
    n_et = len(model._ENT_TABLES)
    q = _QueryRows.apply(model._hip_kind(), side, model._d_ent, model._d_rel, h_idx, t_idx, r_idx, *tables)
    q = q if isinstance(q, tuple) else (q,)
    target = {'tail': t_idx, 'head': h_idx}.get(side)
    if target is None:
        target = torch.cat([t_idx, h_idx])      # tail-side queries first, as lp_problem_both
    return all_candidates_cross_entropy(q, tuple(tables[:n_et]), target, label_smoothing, reduction)
