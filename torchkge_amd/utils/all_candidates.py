# -*- coding: utf-8 -*-
"""What the all-candidates criteria share above their bindings (one_vs_all: softmax cross-entropy, k_vs_all: multi-label
BCE): the KGE_LP_DOT problem of the operands, the checks of the public functions -- the function's name is a parameter of
the messages -- and the frame of the autograd functions' forward and backward."""
import torch

from .. import _hip

REDUCTIONS = ('mean', 'sum', 'none')


def _problem(queries, tables):
    return _hip.LpProblem(_hip.LP_DOT, queries[0], tables[0], A1=queries[1] if len(queries) > 1 else None,
                          T1=tables[1] if len(tables) > 1 else None)


def _segments(fn, x, what):
    xs = (x,) if isinstance(x, torch.Tensor) else tuple(x)
    if not 1 <= len(xs) <= 2:
        raise ValueError('%s: %s is one matrix or a pair of them, got %d' % (fn, what, len(xs)))
    _hip.require_cuda(*xs)
    for m in xs:
        if m.dtype != torch.float32 or m.dim() != 2:
            raise RuntimeError('torchkge_amd: %s expects float32 matrices, got %s of %d dimensions for the %s'
                               % (fn, m.dtype, m.dim(), what))
    return xs


def check_options(fn, label_smoothing, reduction):
    if reduction not in REDUCTIONS:
        raise ValueError("%s: reduction is 'mean', 'sum' or 'none', got %r" % (fn, reduction))
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError('%s: label_smoothing must lie in [0, 1], got %r' % (fn, label_smoothing))


def check_operands(fn, queries, tables, labels):
    """The segment tuples ``(qs, ts)`` of the operands of ``fn``; ``labels``: the label tensors, which must be on the GPU."""
    qs, ts = _segments(fn, queries, 'queries'), _segments(fn, tables, 'tables')
    _hip.require_cuda(*labels)
    if len(qs) != len(ts) or any(q.shape[1] != t.shape[1] for q, t in zip(qs, ts)):
        raise ValueError('%s: queries and tables need the same segments, got widths %s and %s'
                         % (fn, [q.shape[1] for q in qs], [t.shape[1] for t in ts]))
    if any(q.shape[0] != qs[0].shape[0] for q in qs) or any(t.shape[0] != ts[0].shape[0] for t in ts):
        raise ValueError('%s: the segments of one operand need the same number of rows' % fn)
    if ts[0].shape[0] < 1:
        raise ValueError('%s: no candidates' % fn)
    return qs, ts


def forward_problem(ctx, label_smoothing, n_seg, ops):
    """``(ops, prob)``: the operands as float32 rows, detached, and their problem; keeps what ``backward`` reads of ctx."""
    ops = [_hip.f32rows(x.detach()) for x in ops]
    ctx.eps, ctx.n_seg = label_smoothing, n_seg
    return ops, _problem(ops[:n_seg], ops[n_seg:])


def backward(ctx, grad_rows, n_lead, n_saved, bwd):
    """The backward of an autograd function whose inputs are ``n_lead`` non-differentiable ones, then the queries and the
    tables, and whose saved tensors are ``n_saved`` of the criterion's own, then the operands.  ``needs_input_grad``
    decides which products ``bwd(prob, saved, g, want_queries=, want_tables=) -> (dA, dT)`` launches."""
    n = ctx.n_seg
    needs = ctx.needs_input_grad[n_lead:]
    want_q, want_t = any(needs[:n]), any(needs[n:])
    if not (want_q or want_t):
        return (None,) * (n_lead + 2 * n)
    ops = ctx.saved_tensors[n_saved:]
    g = grad_rows.contiguous() if grad_rows.dtype == torch.float32 else grad_rows.float().contiguous()
    dA, dT = bwd(_problem(ops[:n], ops[n:]), ctx.saved_tensors[:n_saved], g, want_queries=want_q, want_tables=want_t)
    grads = list(dA or [None] * n) + list(dT or [None] * n)
    return (None,) * n_lead + tuple(x if need else None for x, need in zip(grads, needs))
