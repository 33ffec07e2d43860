# -*- coding: utf-8 -*-
"""Row-wise optimizers for the row gradients of torchkge_amd.row_gradients().

In row-gradient mode the backward of a scoring function leaves in ``table.grad`` an UNCOALESCED sparse tensor: one
(id, gradient row) pair per triple and operand.  ``step()`` of the optimizers here coalesces those pairs on the device
(kge_rows_coalesce: stable sort, ordered sum, no float atomic -- the same bits on every run) and updates only the rows
that occur (kge_row_sgd / kge_row_adagrad / kge_row_adam, include/kge_hip_rows.h).  The number of distinct rows stays
on the device: nothing here reads back, and no (n_rows, d) gradient exists at any point.  The update rules are those
of the sparse branches of torch.optim.SGD / Adagrad / SparseAdam; state tensors are dense tables, as theirs.

    row_params, dense_params = split_parameters(model)
    opt = RowAdagrad(row_params, lr=0.1)
    opt_dense = torch.optim.Adagrad(dense_params, lr=0.1) if dense_params else None
    with torchkge_amd.row_gradients():
        loss = criterion(*model(h, t, r, nh, nt))
    loss.backward(); opt.step()
"""
import torch
from torch.optim import Optimizer

from . import _hip_rows
from ._hip import require_cuda

__all__ = ['RowSGD', 'RowAdagrad', 'RowAdam', 'coalesce_rows', 'split_parameters']


def coalesce_rows(grad):
    """(uniq, rows, count) of a 2-D sparse COO gradient with dense rows, coalesced or not: the distinct row ids
    ascending, their summed rows (rows[j] belongs to uniq[j]) and the number of distinct ids as a device int64 scalar.
    ``uniq`` and ``rows`` have room for every entry of ``grad``; only their first ``count`` entries mean anything.  No
    host read."""
    if not grad.is_sparse or grad.sparse_dim() != 1 or grad.dense_dim() != 1:
        raise RuntimeError('coalesce_rows: expected a sparse COO gradient of a 2-D table with dense rows')
    ids, vals = grad._indices()[0], grad._values()
    require_cuda(ids, vals)
    if vals.dtype != torch.float32:
        raise RuntimeError('coalesce_rows: expected float32 rows, got %s' % vals.dtype)
    if vals.shape[0] and (vals.stride(1) != 1 or vals.stride(0) < vals.shape[1]):
        vals = vals.contiguous()
    ld = vals.stride(0) if vals.shape[0] > 1 else vals.shape[1]
    return _hip_rows.rows_coalesce(vals, ld, grad.shape[1], ids.contiguous(), grad.shape[0])


def split_parameters(model):
    """(row_params, dense_params) of a model of this package: the embedding tables whose gradient a row-gradient
    backward returns as rows, and every other parameter (RESCAL's rel_mat, TransR's proj_mat, ConvKB's layers), which
    keeps a dense gradient and belongs in a stock optimizer."""
    dense_ids = {id(p) for name in getattr(model, '_DENSE_GRAD_TABLES', ()) for p in getattr(model, name).parameters()}
    row, dense = [], []
    for p in model.parameters():
        is_row = p.dim() == 2 and id(p) not in dense_ids and \
            any(isinstance(m, torch.nn.Embedding) and m.weight is p for m in model.modules())
        (row if is_row else dense).append(p)
    return row, dense


class _RowOptimizer(Optimizer):
    """The shared step: per parameter with a sparse gradient, one kge_rows_coalesce and one update launch."""

    def _check_param(self, p):
        if p.grad.is_sparse:
            if not p.is_cuda or p.dtype != torch.float32 or p.dim() != 2 or not p.is_contiguous():
                raise RuntimeError('%s: a parameter must be a contiguous float32 matrix on the GPU' % type(self).__name__)
            return
        raise RuntimeError('%s got a dense gradient: it updates only parameters with row gradients '
                           '(torchkge_amd.row_gradients()); put this parameter into a stock torch.optim optimizer '
                           '(split_parameters(model) gives the two groups)' % type(self).__name__)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                self._check_param(p)
                uniq, rows, count = coalesce_rows(p.grad)
                self._update(group, p, uniq, rows, count)
        return loss


class RowSGD(_RowOptimizer):
    """torch.optim.SGD's sparse step (no momentum, no weight decay) on the touched rows: p -= lr * g."""

    def __init__(self, params, lr):
        if not lr >= 0.0:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        super().__init__(params, dict(lr=lr))

    def _update(self, group, p, uniq, rows, count):
        _hip_rows.row_sgd(p, uniq, count, rows, group['lr'])


class RowAdagrad(_RowOptimizer):
    """torch.optim.Adagrad's sparse step on the touched rows: sum += g^2; p -= clr * g / (sqrt(sum) + eps) with
    clr = lr / (1 + (step - 1) * lr_decay).  State: ``sum`` (a dense table) and ``step``."""

    def __init__(self, params, lr, lr_decay=0, eps=1e-10, initial_accumulator_value=0):
        if not lr >= 0.0:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not lr_decay >= 0.0:
            raise ValueError('Invalid lr_decay value: %r' % (lr_decay,))
        if not eps >= 0.0:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not initial_accumulator_value >= 0.0:
            raise ValueError('Invalid initial_accumulator_value value: %r' % (initial_accumulator_value,))
        super().__init__(params, dict(lr=lr, lr_decay=lr_decay, eps=eps, initial_accumulator_value=initial_accumulator_value))

    def _update(self, group, p, uniq, rows, count):
        state = self.state[p]
        if not state:
            state['step'] = 0
            state['sum'] = torch.full_like(p, group['initial_accumulator_value'], memory_format=torch.contiguous_format)
        state['step'] += 1
        clr = group['lr'] / (1 + (state['step'] - 1) * group['lr_decay'])
        _hip_rows.row_adagrad(p, state['sum'], uniq, count, rows, clr, group['eps'])


class RowAdam(_RowOptimizer):
    """torch.optim.SparseAdam's lazy step on the touched rows: the moments of rows without a gradient do not decay,
    the bias correction uses the global step.  State: ``exp_avg``, ``exp_avg_sq`` (dense tables) and ``step``."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8):
        if not lr > 0.0:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not eps > 0.0:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError('Invalid beta parameter at index 0: %r' % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError('Invalid beta parameter at index 1: %r' % (betas[1],))
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))

    def _update(self, group, p, uniq, rows, count):
        state = self.state[p]
        if not state:
            state['step'] = 0
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        state['step'] += 1
        beta1, beta2 = group['betas']
        _hip_rows.row_adam(p, state['exp_avg'], state['exp_avg_sq'], uniq, count, rows, group['lr'], beta1, beta2,
                           group['eps'], state['step'])
