"""The yardstick of the embedding regularizers (include/kge_hip_penalty.h), TEST ONLY: the penalty's formulas in float64
on the fp32 tables, closed-form gradients (``torch.sqrt(re ** 2 + im ** 2) ** 3`` has a NaN autograd gradient at 0; the
closed form p |x| ** (p - 2) x is 0 there), and autograd on top of the closed-form terms for whole-model checks."""
import torch

REAL, SPLIT, INTERLEAVED = 0, 1, 2


def row_power_sums(layout, p, t0, t1=None):
    """sum_k |x_k| ** p of every row, float64: (rows,)."""
    x0 = t0.double()
    if layout == REAL:
        return x0.abs().pow(p).sum(1)
    re, im = (x0, t1.double()) if layout == SPLIT else (x0[:, 0::2], x0[:, 1::2])
    m2 = re * re + im * im
    return (m2 if p == 2 else m2 * m2.sqrt()).sum(1)


def row_gradients(layout, p, t0, t1=None):
    """d (sum_k |x_k| ** p) / d row, float64, closed form: one matrix, for SPLIT the pair (d / d re, d / d im)."""
    x0 = t0.double()
    if layout == REAL:
        return p * x0.abs().pow(p - 2) * x0
    if layout == SPLIT:
        re, im = x0, t1.double()
        s = p * (re * re + im * im).sqrt().pow(p - 2)
        return s * re, s * im
    re, im = x0[:, 0::2], x0[:, 1::2]
    s = p * (re * re + im * im).sqrt().pow(p - 2)
    return torch.stack([s * re, s * im], dim=2).reshape(x0.shape)


def terms(streams, p):
    """The M per-occurrence terms of ``streams`` -- tuples (layout, t0, t1, ids, factor) -- in float64, the factor as the
    fp32 number the kernel takes."""
    out = []
    for layout, t0, t1, ids, factor in streams:
        f = torch.tensor(factor, dtype=torch.float32).double().item()
        out.append(f * row_power_sums(layout, p, t0, t1)[ids])
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64)


def gradient_rows(streams, p, go=1.0):
    """The rows buffer of kge_row_penalty_bwd in float64, block by block in the header's layout, flattened."""
    out = []
    for layout, t0, t1, ids, factor in streams:
        f = torch.tensor(factor, dtype=torch.float32).double().item() * go
        g = row_gradients(layout, p, t0, t1)
        for block in (g if layout == SPLIT else (g,)):
            out.append((f * block[ids]).reshape(-1))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64)


N_ENT, N_REL = 50, 5


def zoo(d):
    """name -> (constructor of a small model of width d, its expected groups): per side a list of (layout, parameter
    name or pair of names).  Every model class of the package."""
    from torchkge_amd import models as M
    e, r = [(REAL, 'ent_emb')], [(REAL, 'rel_emb')]
    return {
        'TransE': (lambda: M.TransEModel(d, N_ENT, N_REL, 'L2'), (e, r)),
        'TorusE': (lambda: M.TorusEModel(d, N_ENT, N_REL, 'torus_L2'), (e, r)),
        'TransH': (lambda: M.TransHModel(d, N_ENT, N_REL), (e, r + [(REAL, 'norm_vect')])),
        'TransD': (lambda: M.TransDModel(d, d, N_ENT, N_REL), (e + [(REAL, 'ent_proj_vect')], r + [(REAL, 'rel_proj_vect')])),
        'TransR': (lambda: M.TransRModel(d, d + 1, N_ENT, N_REL), (e, r + [(REAL, 'proj_mat')])),
        'RotatE': (lambda: M.RotatEModel(d, N_ENT, N_REL), ([(INTERLEAVED, 'ent_emb')], [])),
        'DistMult': (lambda: M.DistMultModel(d, N_ENT, N_REL), (e, r)),
        'ComplEx': (lambda: M.ComplExModel(d, N_ENT, N_REL), ([(SPLIT, ('re_ent_emb', 'im_ent_emb'))],
                                                               [(SPLIT, ('re_rel_emb', 'im_rel_emb'))])),
        'RESCAL': (lambda: M.RESCALModel(d, N_ENT, N_REL), (e, [(REAL, 'rel_mat')])),
        'HolE': (lambda: M.HolEModel(d, N_ENT, N_REL), (e, r)),
        'ANALOGY': (lambda: M.AnalogyModel(d, N_ENT, N_REL), ([(REAL, 'sc_ent_emb'), (SPLIT, ('re_ent_emb', 'im_ent_emb'))],
                                                               [(REAL, 'sc_rel_emb'), (SPLIT, ('re_rel_emb', 'im_rel_emb'))])),
        'ConvKB': (lambda: M.ConvKBModel(d, 3, N_ENT, N_REL), (e, r)),
    }


class _Power(torch.autograd.Function):
    """sum_k |x_k| ** p of every row with the closed-form backward: differentiable at 0."""

    @staticmethod
    def forward(ctx, layout, p, t0, t1):
        ctx.layout, ctx.p = layout, p
        ctx.save_for_backward(t0, t1)
        return row_power_sums(layout, p, t0, t1)

    @staticmethod
    def backward(ctx, go):
        t0, t1 = ctx.saved_tensors
        g = row_gradients(ctx.layout, ctx.p, t0, t1)
        if ctx.layout == SPLIT:
            return None, None, go.view(-1, 1) * g[0], go.view(-1, 1) * g[1]
        return None, None, go.view(-1, 1) * g, None


def penalty64(groups, p, weights, ids):
    """The penalty of a model in float64 with autograd: ``groups`` = (entity groups, relation groups) of float64 leaf
    tables as (layout, t0, t1), ``weights`` = (entity weight, relation weight), ``ids`` = (entity id vectors, relation
    id vectors).  Every group with every id vector of its side, per occurrence, w / n each -- w / n as the fp32 number
    the engine is handed."""
    total = torch.zeros((), dtype=torch.float64, device=ids[0][0].device)
    for side, w, vectors in zip(groups, weights, ids):
        for layout, t0, t1 in side:
            sums = _Power.apply(layout, p, t0, t1)
            for v in vectors:
                f = torch.tensor(w / v.shape[0], dtype=torch.float32).double().item()
                total = total + f * sums[v].sum()
    return total
