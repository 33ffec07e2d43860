"""The float64 forms of include/kge_hip_bce.h on the CPU, built from a score matrix taken as given and a dense label
matrix scattered from the CSR.  Test-only."""
import torch


def _s64(S):
    return S.detach().double().cpu()


def dense_labels(seg_lo, seg_hi, targets, N):
    """(B, N) float64 0/1 matrix: row i holds ones at targets[seg_lo[i]:seg_hi[i]]."""
    lo, hi, tg = (x.detach().cpu().long() for x in (seg_lo, seg_hi, targets))
    Y = torch.zeros(lo.shape[0], N, dtype=torch.float64)
    for i in range(lo.shape[0]):
        if hi[i] > lo[i]:
            Y[i, tg[lo[i]:hi[i]]] = 1.0
    return Y


def smooth(Y, eps):
    """y = (1 - eps) [c in set] + eps / N: every label mixed with the uniform distribution over the N candidates."""
    return (1.0 - eps) * Y + eps / Y.shape[1]


def row_loss64(S, Y, eps=0.0):
    """row_loss_i = sum_c [ softplus(s) - y s ],  softplus(s) = max(s, 0) + log1p(exp(-|s|))."""
    S = _s64(S)
    return (S.clamp(min=0) + torch.log1p((-S.abs()).exp()) - smooth(Y, eps) * S).sum(dim=1)


def g_matrix64(S, Y, eps, g):
    """G(i, c) = g_i (sigma(s) - y)."""
    S = _s64(S)
    return g.detach().double().cpu().view(-1, 1) * (torch.sigmoid(S) - smooth(Y, eps))


def grads64(S, Y, eps, g, A, T):
    """(dA, dT) = (G . T, G^T . A) in float64; A, T: the operands (segments already concatenated along K)."""
    G = g_matrix64(S, Y, eps, g)
    return G @ T.detach().double().cpu(), G.t() @ A.detach().double().cpu()
