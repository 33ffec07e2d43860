# -*- coding: utf-8 -*-
"""Embedding regularizers on the HIP engine (include/kge_hip_penalty.h): the penalties the published recipes of the
training regimes carry -- N3 for ComplEx / DistMult trained 1-vs-all (Lacroix et al. 2018), squared L2 for the older runs,
the L3 penalty of the RotatE code base -- as one gather of the penalised rows, a fixed-order sum and gradient ROWS.

    reg = N3Regularizer(weight=0.05)
    loss = criterion(pos, neg) + reg(model, (h, t), (r,))
    trainer.regularizer = reg           # Trainer, OneVsAllTrainer, KvsAllTrainer: an attribute, None by default

For a batch, with p in {2, 3}:

    penalty = sum over the streams s of (w_s / n_s) * sum_{i < n_s} sum_k |x_{s,i,k}| ** p

A stream is one table (or one complex pair of tables) of the model gathered by one id vector of n_s ids; w_s is the entity
weight or the relation weight.  The sum is per occurrence -- a row that occurs twice is penalised twice, the frequency
weighting of Lacroix et al. -- and over the rows as stored, before any normalisation a scorer applies.

What a penalty written in torch on ``model.ent_emb(h)`` cannot give: the gradient of a table is the sum of gradient rows
through the reduction every other backward uses (ordered inside ``deterministic()``), or, inside ``row_gradients()``, a
sparse row gradient that ``RowSGD`` / ``RowAdagrad`` / ``RowAdam`` step on; no table-sized tensor exists unless the
optimizer asks for a dense gradient."""
import torch

from .. import _hip, _hip_penalty


def _vectors(ids):
    return [ids] if torch.is_tensor(ids) else list(ids)


class LpRegularizer(object):
    """``LpRegularizer(p=3, weight=0.01, relation_weight=None, modulus=True)``: the Lp penalty, ``p`` 2 or 3, of the rows
    of a model's embedding tables that a batch names.  ``weight``: the entity weight; ``relation_weight``: None takes
    ``weight``.  ``modulus=True`` penalises a complex coordinate (ComplEx, ANALOGY's complex part, RotatE's entities) by
    its modulus sqrt(re ** 2 + im ** 2); ``modulus=False`` treats every table element by element.  For p = 2 the two
    coincide.  p = 1 is left out: it has a kink and no recipe uses it.

    ``reg(model, entity_ids, relation_ids, acc=None)`` returns the penalty as a float32 device scalar, differentiable with
    respect to the model's tables.  Each ids argument is a tensor or a sequence of tensors -- ``(h, t)``, ``(r,)``; every
    entity group of ``model._penalty_groups()`` is paired with every entity id vector, likewise for relations.  ``acc``:
    a float32 device scalar the penalty is also added to.  A row-sharded model raises."""

    def __init__(self, p=3, weight=0.01, relation_weight=None, modulus=True):
        if p not in (2, 3):
            raise ValueError('torchkge_amd: an Lp regularizer takes p = 2 or p = 3, got %r' % (p,))
        self.p = int(p)
        self.weight = float(weight)
        self.relation_weight = self.weight if relation_weight is None else float(relation_weight)
        self.modulus = bool(modulus)

    def _groups(self, model):
        """The model's groups as ``(layout, t0, t1)``; ``modulus=False``: every table a REAL group of its own."""
        out = []
        for groups in model._penalty_groups():
            side = []
            for layout, tabs in groups:
                tabs = tuple(tabs) if isinstance(tabs, (tuple, list)) else (tabs,)
                if self.modulus:
                    side.append((layout, tabs[0], tabs[1] if len(tabs) > 1 else None))
                else:
                    side += [(_hip_penalty.REAL, x, None) for x in tabs]
            out.append([g for g in side if g[1].shape[1] > 0])
        return out

    def __call__(self, model, entity_ids, relation_ids, acc=None):
        model._check_unsharded('an embedding regularizer')
        ent, rel = self._groups(model)
        ids, tables, pos, spec = [], [], {}, []

        def table(x):
            if id(x) not in pos:
                pos[id(x)] = len(tables)
                tables.append(x)
            return pos[id(x)]

        for groups, vectors, w in ((ent, _vectors(entity_ids), self.weight), (rel, _vectors(relation_ids), self.relation_weight)):
            for v in vectors:
                ids.append(v)
            for layout, t0, t1 in groups:
                for k in range(len(ids) - len(vectors), len(ids)):
                    n = ids[k].shape[0]
                    if n and w != 0.0:
                        spec.append((layout, table(t0), None if t1 is None else table(t1), k, w / n))
        _hip.require_cuda(*(ids + tables))
        if not spec:
            dev = tables[0].device if tables else (ids[0].device if ids else 'cuda')
            return torch.zeros((), dtype=torch.float32, device=dev)
        by_id = {id(getattr(model, n).weight) for n in model._DENSE_GRAD_TABLES}
        dense = frozenset(i for i, x in enumerate(tables) if id(x) in by_id)
        total = None
        for q in range(0, len(spec), _hip_penalty.MAX_STREAMS):     # (ANALOGY element by element: nine streams)
            part = _hip_penalty.RowPenalty.apply(self.p, tuple(spec[q:q + _hip_penalty.MAX_STREAMS]), dense, acc, len(ids),
                                                 *(ids + tables))
            total = part if total is None else total + part
        return total


class N3Regularizer(LpRegularizer):
    """``N3Regularizer(weight, relation_weight=None)``: the nuclear 3-norm penalty of Lacroix et al. 2018 --
    ``LpRegularizer(p=3, modulus=True)``."""

    def __init__(self, weight, relation_weight=None):
        super().__init__(p=3, weight=weight, relation_weight=relation_weight, modulus=True)
