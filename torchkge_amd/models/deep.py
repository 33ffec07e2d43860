# -*- coding: utf-8 -*-
"""ConvKB (torchkge/models/deep.py:13-154) on the HIP engine.

The reference pushes a (b * N, 3, d) candidate tensor through Conv1d -> ReLU -> Linear -> Softmax: an activation of
b * N * F * d floats.  Here the same numbers come from registers (include/kge_hip_convkb.h: the closed form on
D = L[1] - L[0], one accumulator per pair) and that tensor is never written."""
import torch
from torch import nn

from .. import _hip, _hip_convkb
from ..rowgrad import is_row_gradients
from ..utils.modeling import init_embedding
from .interfaces import Model


class _ConvKBScore(torch.autograd.Function):
    """ConvKB's scoring_function over kge_convkb_score_triples / _bwd, differentiable in all six parameters."""

    @staticmethod
    def forward(ctx, d, F, h, t, r, ent, rel, conv_w, conv_b, lin_w, lin_b):
        ent, rel, conv_w, conv_b, lin_w, lin_b = (x.detach() for x in (ent, rel, conv_w, conv_b, lin_w, lin_b))
        ws = _hip_convkb.prepare(conv_w, conv_b, lin_w, lin_b, d)
        s = _hip_convkb.score_triples(ent, rel, ws, d, F, h, t, r)
        ctx.d, ctx.F = d, F
        ctx.row_grads = is_row_gradients()      # read here: a loss built inside row_gradients() keeps the mode
        ctx.save_for_backward(h, t, r, ent, rel, ws, s)
        return s

    @staticmethod
    def backward(ctx, grad_out):
        h, t, r, ent, rel, ws, s = ctx.saved_tensors
        grads = _hip_convkb.score_triples_bwd(ent, rel, ws, ctx.d, ctx.F, h, t, r, s, grad_out, ctx.needs_input_grad[5:],
                                              row_grads=ctx.row_grads)
        return (None,) * 5 + tuple(grads)


def _table4_of(cand):
    """(N, d) table if ``cand`` is the batch-broadcast (stride-0) (b, N, 1, d) view inference_prepare_candidates returns
    (or has a single batch row), else None."""
    if torch.is_tensor(cand) and cand.dim() == 4 and cand.shape[2] == 1 and cand.stride(3) == 1 and \
            (cand.stride(0) == 0 or cand.shape[0] == 1):
        return cand[0, :, 0, :]
    return None


class ConvKBModel(Model):
    """ConvKB (deep.py:13-154): ``ConvKBModel(emb_dim, n_filters, n_entities, n_relations)``; parameters ``ent_emb``,
    ``rel_emb``, ``convlayer.0`` (Conv1d(3, n_filters, 1)) and ``output.0`` (Linear(emb_dim * n_filters, 2)) in the
    reference's module tree, so a reference checkpoint loads.  score = softmax(output(relu(conv([h; r; t]))))[1].

    The two Sequentials only HOLD the parameters: every score comes from the kernels of csrc/convkb.hip.  All-candidates
    scores, fused rank counts and the filter correction run on ``_hip_convkb.ConvKBProblem``; there is no f16 prefilter
    for this score (``split_filter = False``: no guard vector).  Row-sharded entity tables are out of scope."""

    _kind = None            # no kind of include/kge_hip.h: the entry points are those of include/kge_hip_convkb.h
    _ENT_TABLES = ('ent_emb',)
    lp_dedupe_queries = False       # the count sweeps queries, not distinct query rows: ``cols`` is ignored

    def __init__(self, emb_dim, n_filters, n_entities, n_relations):
        super().__init__(n_entities, n_relations)
        self.emb_dim = emb_dim
        self.n_filters = n_filters
        _hip_convkb.check_dims(emb_dim, n_filters)
        self.split_filter = False
        self.ent_emb = init_embedding(self.n_ent, self.emb_dim)
        self.rel_emb = init_embedding(self.n_rel, self.emb_dim)
        self.convlayer = nn.Sequential(nn.Conv1d(3, n_filters, 1, stride=1), nn.ReLU())
        self.output = nn.Sequential(nn.Linear(emb_dim * n_filters, 2), nn.Softmax(dim=1))

    def _tables(self):
        return [self.ent_emb.weight, self.rel_emb.weight] + self._layer_params()

    def _layer_params(self):
        return [self.convlayer[0].weight, self.convlayer[0].bias, self.output[0].weight, self.output[0].bias]

    def _uses_guard(self):
        return False

    # ---- row sharding: out of scope ------------------------------------------
    def shard_entities_(self, lo, hi):
        raise RuntimeError('torchkge_amd: row-sharded entity tables are out of scope for ConvKBModel')

    def as_entity_shard_(self, n_total, lo, hi):
        raise RuntimeError('torchkge_amd: row-sharded entity tables are out of scope for ConvKBModel')

    # ---- reference API -------------------------------------------------------
    def scoring_function(self, h_idx, t_idx, r_idx):
        """Score of each triplet (deep.py:63-77): two launches (layer preparation, fused gather + score), differentiable."""
        tables = self._tables()
        _hip.require_cuda(h_idx, t_idx, r_idx, *tables)
        return _ConvKBScore.apply(self.emb_dim, self.n_filters, h_idx, t_idx, r_idx, *tables)

    def normalize_parameters(self):
        """No normalisation for ConvKB (deep.py:79-85)."""
        pass

    def get_embeddings(self):
        """(ent_emb, rel_emb) (deep.py:87-99)."""
        self.normalize_parameters()
        return self.ent_emb.weight.data, self.rel_emb.weight.data

    # ---- the prepared layer ----------------------------------------------------
    def _prepared(self):
        """kge_convkb_prepare's workspace of the four layer parameters: built once per lp_session (never kept across
        sessions: the weights may change between them); inside a captured evaluation the launch is part of the graph
        and reads the parameters at their addresses, so a replay follows in-place updates."""
        layer = [x.data for x in self._layer_params()]
        return self._cache.get('ckb_ws', layer, lambda: _hip_convkb.prepare(*layer, self.emb_dim))

    def _problem(self, slot, QE, qe_idx, QR, qr_idx, T, B, c_base=0, B_tail=0):
        return _hip_convkb.ConvKBProblem(slot, QE, qe_idx, QR, qr_idx, T, self._prepared(), self.emb_dim, self.n_filters,
                                         B, c_base=c_base, B_tail=B_tail)

    def inference_scoring_function(self, h, t, r):
        """Scores against every candidate; the 4-D argument is the candidate set (deep.py:101-130).  A broadcast view of
        a table (what inference_prepare_candidates returns) goes to the tile kernel; a materialised (b, N, 1, d) tensor
        is scored pair by pair."""
        A = _hip_convkb
        if t.dim() == 4:
            assert h.dim() == 2 and r.dim() == 2        # tail completion
            slot, qe, qr, cand = A.SLOT_TAIL, h, r, t
        elif h.dim() == 4:
            assert t.dim() == 2 and r.dim() == 2        # head completion
            slot, qe, qr, cand = A.SLOT_HEAD, t, r, h
        else:
            assert r.dim() == 4 and h.dim() == 2 and t.dim() == 2       # relation prediction
            slot, qe, qr, cand = A.SLOT_REL, h, t, r
        b = qe.shape[0]
        table = _table4_of(cand)
        if table is not None:
            return self._problem(slot, qe, None, qr, None, table, b).scores()
        # real materialised candidates: row (i, c) of the flattened tensor is candidate i * N + c of query i
        n = cand.shape[1]
        flat = cand.reshape(b * n, self.emb_dim)
        ci = torch.arange(b * n, device=flat.device)
        qi = torch.arange(b, device=flat.device).repeat_interleave(n)
        return self._problem(slot, qe, None, qr, None, flat, b).pair_scores(ci, qi).view(b, n)

    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """(h, t, r, candidates): gathered rows and the stride-0 (b, N, 1, d) view of the entity table (``entities=False``:
        of the relation table) (deep.py:132-154)."""
        b_size = max(h_idx.shape[0], t_idx.shape[0], r_idx.shape[0])   # inference passes one empty index
        ent, rel = self.ent_emb.weight.data, self.rel_emb.weight.data
        _hip.require_cuda(h_idx, t_idx, r_idx, ent, rel)
        h, t, r = _hip.gather_rows(ent, h_idx), _hip.gather_rows(ent, t_idx), _hip.gather_rows(rel, r_idx)
        src, n = (ent, self.n_ent) if entities else (rel, self.n_rel)
        cand = src.view(1, n, self.emb_dim).expand(b_size, n, self.emb_dim).view(b_size, n, 1, self.emb_dim)
        return h, t, r, cand

    # ---- evaluation ---------------------------------------------------------
    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        """ConvKBProblem of one batch straight from index vectors, over table rows [ent_lo, ent_hi): 'tail', 'head', or
        'both' (2B queries, tail side first).  ``cols`` is ignored (lp_dedupe_queries = False)."""
        if exchange is not None or qtabs is not None:
            raise RuntimeError('torchkge_amd: row-sharded entity tables are out of scope for ConvKBModel')
        ent_hi = self.n_ent if ent_hi is None else ent_hi
        ent, rel = self.ent_emb.weight.data, self.rel_emb.weight.data
        T = ent if (ent_lo == 0 and ent_hi == ent.shape[0]) else ent[ent_lo:ent_hi]
        A = _hip_convkb
        b = r_idx.shape[0]
        if side == 'tail':
            return self._problem(A.SLOT_TAIL, ent, h_idx, rel, r_idx, T, b, c_base=ent_lo)
        if side == 'head':
            return self._problem(A.SLOT_HEAD, ent, t_idx, rel, r_idx, T, b, c_base=ent_lo)
        assert side == 'both'
        r_both = self._lp_r_both if self._lp_r_both is not None else torch.cat([r_idx, r_idx])
        return self._problem(A.SLOT_BOTH, ent, torch.cat([h_idx, t_idx]), rel, r_both, T, 2 * b, c_base=ent_lo, B_tail=b)
