"""float64 restatement of RotatE on interleaved tables (test-only): E (n_ent, 2d) rows are (re_0, im_0, re_1, im_1, ...),
P (n_rel, d) phases in radians; score(h, r, t) = -sum_k |h_k exp(i theta_k) - t_k|.  Everything here takes the fp32
tables the engine holds and computes in float64 / complex128."""
import torch


def as_complex(E):
    """(rows, 2d) interleaved real table -> (rows, d) complex128."""
    E = torch.as_tensor(E).double().contiguous()
    return torch.view_as_complex(E.view(E.shape[0], E.shape[1] // 2, 2))


def rotation(P):
    """exp(i theta), complex128."""
    P = torch.as_tensor(P).double()
    return torch.polar(torch.ones_like(P), P)


def cmod_scores64(Q, T):
    """KGE_LP_CMOD in float64 on the SAME fp32 operands: s[i, c] = -sum_j |(Q[i] - T[c])_j| over the interleaved pairs."""
    return -(as_complex(Q).unsqueeze(1) - as_complex(T).unsqueeze(0)).abs().sum(-1)


def sf64(E, P, h, t, r):
    """scoring_function: -sum_k |h_k r_k - t_k|."""
    Ec, R = as_complex(E), rotation(P)
    return -(Ec[h] * R[r] - Ec[t]).abs().sum(-1)


def queries64(E, P, h, t, r, side):
    """Query rows as complex128: tail side h o r, head side t o conj(r)."""
    Ec, R = as_complex(E), rotation(P)
    return Ec[h] * R[r] if side == 'tail' else Ec[t] * R[r].conj()


def scores64(E, P, h, t, r, side, chunk=64):
    """(b, N) all-candidates scores from the DEFINITION: tail side -|h r - c|, head side -|c r - t| (summed over k)."""
    Ec, R = as_complex(E), rotation(P)
    out = []
    for c0 in range(0, h.shape[0], chunk):
        sl = slice(c0, c0 + chunk)
        if side == 'tail':
            y = (Ec[h[sl]] * R[r[sl]]).unsqueeze(1) - Ec.unsqueeze(0)
        else:
            y = Ec.unsqueeze(0) * R[r[sl]].unsqueeze(1) - Ec[t[sl]].unsqueeze(1)
        out.append(-y.abs().sum(-1))
    return torch.cat(out) if out else torch.zeros(0, Ec.shape[0], dtype=torch.float64)


def relation_scores64(E, P, h, t):
    """(b, n_rel): -sum_k |h_k r_ck - t_k| for every relation c."""
    Ec, R = as_complex(E), rotation(P)
    return -(Ec[h].unsqueeze(1) * R.unsqueeze(0) - Ec[t].unsqueeze(1)).abs().sum(-1)


def grads64(E, P, h, t, r, go):
    """float64 autograd of sum_i go_i * -(h * polar(1, theta) - t).abs().sum(-1): (dE interleaved (n_ent, 2d), dP)."""
    E64 = torch.as_tensor(E).double().clone().requires_grad_()
    P64 = torch.as_tensor(P).double().clone().requires_grad_()
    Ec = torch.view_as_complex(E64.view(E64.shape[0], -1, 2))
    s = -(Ec[h] * torch.polar(torch.ones_like(P64[r]), P64[r]) - Ec[t]).abs().sum(-1)
    (s * torch.as_tensor(go).double()).sum().backward()
    return E64.grad, P64.grad
