"""The yardstick of the grouped criteria (include/kge_hip_group.h): the header's forms in float64 torch on the CPU, and
the same criteria written out with torch's stock operators (what a user writes today; the fp32 comparator of the GPU
tests and the float64 anchor of the host test).  Test-only."""
import torch
import torch.nn.functional as F

KINDS = ('nssa', 'softmax')


def softplus64(x):
    return x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))


def sigma64(x):
    e = torch.exp(-x.abs())
    return torch.where(x >= 0, 1 / (1 + e), e / (1 + e))


def forms64(kind, margin, temperature, pos, neg, weights=None):
    """(row_loss, loss, dpos, dneg) of the header's table in float64 on the CPU.  pos: (B) scores, neg: (K, B), taken as
    they are (fp32 values widened); weights: (B) or None."""
    p, x = pos.detach().double().cpu(), neg.detach().double().cpu()
    assert x.dim() == 2 and x.shape[1] == p.shape[0]
    if kind == 'nssa':
        u = float(temperature) * x
        m = u.max(dim=0, keepdim=True).values
        e = torch.exp(u - m)
        w = e / e.sum(dim=0, keepdim=True)
        row = softplus64(-(margin + p)) + (w * softplus64(margin + x)).sum(dim=0)
        dp = -sigma64(-(margin + p))
        dn = w * sigma64(margin + x)
    else:
        allx = torch.cat([p.view(1, -1), x])
        m = allx.max(dim=0).values
        lse = m + torch.log(torch.exp(allx - m).sum(dim=0))
        row = lse - p
        dp = torch.exp(p - lse) - 1
        dn = torch.exp(x - lse)
    if weights is not None:
        wt = weights.detach().double().cpu()
        row, dp, dn = row * wt, dp * wt, dn * wt
    return row, row.sum(), dp, dn


def written_out(kind, margin, temperature, pos, neg, weights=None):
    """The criterion with torch's stock operators, in the dtype and on the device of the scores: the per-fact terms (B).
    pos: (B), neg: (K, B); differentiable."""
    if kind == 'nssa':
        w = F.softmax(temperature * neg, dim=0).detach()
        row = -F.logsigmoid(margin + pos) - (w * F.logsigmoid(-(margin + neg))).sum(dim=0)
    else:
        scores = torch.cat([pos.view(-1, 1), neg.t()], dim=1)           # (B, K + 1), the fact in column 0
        row = F.cross_entropy(scores, torch.zeros(pos.shape[0], dtype=torch.long, device=pos.device), reduction='none')
    return row if weights is None else row * weights


def stock(kind, margin, temperature, pos, neg, weights=None):
    """(row_loss, loss, dpos, dneg) of ``written_out`` with autograd gradients, detached."""
    p, x = pos.detach().clone().requires_grad_(), neg.detach().clone().requires_grad_()
    row = written_out(kind, margin, temperature, p, x, weights)
    loss = row.sum()
    loss.backward()
    return row.detach(), loss.detach(), p.grad, x.grad
