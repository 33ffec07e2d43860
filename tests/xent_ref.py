"""The float64 forms of include/kge_hip_xent.h on the CPU, built from a score matrix taken as given.  Test-only."""
import torch


def _s64(S):
    return S.detach().double().cpu()


def lse64(S):
    """lse_i = m_i + log(sum_c exp(s(i, c) - m_i))."""
    S = _s64(S)
    m = S.max(dim=1, keepdim=True).values
    return (m + (S - m).exp().sum(dim=1, keepdim=True).log()).view(-1)


def row_loss64(S, target, eps=0.0):
    """(lse, row_loss): row_loss_i = (1 - eps)(lse_i - s(i, t_i)) + eps (lse_i - mean_c s(i, c))."""
    S, t = _s64(S), target.detach().cpu().long()
    lse = lse64(S)
    st = S.gather(1, t.view(-1, 1)).view(-1)
    return lse, (1.0 - eps) * (lse - st) + eps * (lse - S.mean(dim=1))


def g_matrix64(S, target, eps, g, lse=None):
    """G(i, c) = g_i (exp(s(i, c) - lse_i) - (1 - eps)[c = t_i] - eps / N); ``lse``: the one to use (float64 of S: None)."""
    S, t = _s64(S), target.detach().cpu().long()
    lse = lse64(S) if lse is None else lse.detach().double().cpu()
    onehot = torch.zeros_like(S)
    onehot.scatter_(1, t.view(-1, 1), 1.0)
    return g.detach().double().cpu().view(-1, 1) * ((S - lse.view(-1, 1)).exp() - (1.0 - eps) * onehot - eps / S.shape[1])


def grads64(S, target, eps, g, A, T, lse=None):
    """(dA, dT) = (G . T, G^T . A) in float64; A, T: the operands (segments already concatenated along K)."""
    G = g_matrix64(S, target, eps, g, lse)
    return G @ T.detach().double().cpu(), G.t() @ A.detach().double().cpu()
