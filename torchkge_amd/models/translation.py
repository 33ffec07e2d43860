# -*- coding: utf-8 -*-
"""TransE / TransH / TransR / TransD / TorusE with the reference's constructors, attributes and
state_dict keys (torchkge/models/translation.py:18-767) on the HIP engine, and RotatE, which the
reference does not have.

TransH / TransD never build the reference's (n_rel, n_ent, d) projection cache
(`projected_entities`, filled by an n_ent-iteration Python loop,
translation.py:260-284 / :629-652): one scalar per (entity, relation) [TransH:
a = E.W^T] or per entity [TransD: s = Ep.E] is enough, and the rank-1
correction is applied inside the all-candidates kernel.  TransR (:432-458)
likewise: Z[r, c] = ||M_r e_c||^2 is all its cache is needed for.
"""
import math
import os

import torch

from .. import _hip, _hip_rotate
from ..exceptions import NotYetImplementedError
from ..utils.modeling import init_embedding
from .interfaces import Model, TranslationModel, EntityCandidates, RelationProjections, _table_of, _ScoreTriples
from .interfaces import guard_slot, G_QMAX, G_EMAX, G_XABS, G_YABS


def _projections(kind, tabs, d_ent, d_rel, h_idx, t_idx, r_idx):
    """p_r(h), p_r(t) for the index vectors that are present (top-k inference
    passes an empty tensor for the missing side, inference.py:230-238)."""
    empty = torch.zeros(0, d_rel, dtype=torch.float32, device=r_idx.device)
    any_idx = h_idx if h_idx.shape[0] else t_idx
    proj_h = _hip.lp_prep(kind, _hip.SIDE_PROJ_H, tabs, d_ent, d_rel, h_idx, any_idx, r_idx, want_w=True)[0] \
        if h_idx.shape[0] else empty
    proj_t = _hip.lp_prep(kind, _hip.SIDE_PROJ_T, tabs, d_ent, d_rel, any_idx, t_idx, r_idx, want_w=True)[0] \
        if t_idx.shape[0] else empty
    return proj_h, proj_t


def _shard(table, lo, hi):
    return table if (lo == 0 and hi == table.shape[0]) else table[lo:hi]


def _ent_range(model, ent_lo, ent_hi):
    """Default candidate range: the whole table -- or, for a row-sharded model, its own rows."""
    if ent_hi is None:
        return model._row_shard if model._row_shard is not None else (0, model.n_ent)
    return ent_lo, ent_hi


class TransEModel(TranslationModel):
    """TransE (translation.py:18-125).  ``TransEModel(emb_dim, n_entities,
    n_relations, dissimilarity_type='L2')``; parameters ``ent_emb``, ``rel_emb``."""

    def __init__(self, emb_dim, n_entities, n_relations, dissimilarity_type='L2'):
        super().__init__(n_entities, n_relations, dissimilarity_type)
        self.emb_dim = emb_dim
        self.ent_emb = init_embedding(self.n_ent, self.emb_dim)
        self.rel_emb = init_embedding(self.n_rel, self.emb_dim)
        # translation.py:66-67: entities and (once) relations L2-normalised
        self.ent_emb.weight.data = torch.nn.functional.normalize(self.ent_emb.weight.data, p=2, dim=1)
        self.rel_emb.weight.data = torch.nn.functional.normalize(self.rel_emb.weight.data, p=2, dim=1)
        self._sad_bounds = self._abs_bounds

    _ENT_TABLES = ('ent_emb',)
    # the evaluator may hand lp_problem(side='both') a ColumnPlan: the fused query pipeline then writes one split row
    # per DISTINCT query row of the batch and the count kernel sweeps columns instead of queries
    lp_dedupe_queries = True
    # ... but not on the one-product level of the split prefilter: at d = 200 a shared row saves 4 MFMA groups per tile,
    # less than the grouped columns' multi-pass epilogue costs (r04 kernel: 0.632 vs 0.648 ms per evaluate).  r06 taught the
    # free-running kernel grouped columns (lp_hi_stream_kernel<.., GS = 4>) and measured again, same box, alternating: per
    # query 0.487-0.491 ms, columns 0.532-0.544 (profiles/r06/dedupe_level1_stream_ab.txt: the single-query launch 187 us +
    # the grouped one 104 us -- 57 panels, 6 items per workgroup, 2.85 compare passes per column -- against 283 us for the
    # per-query sweep; -24 % MFMAs do not pay on a kernel whose matrix pipe is 42 % busy).  KGE_TRANSE_DEDUPE_L1=1 turns it on.
    lp_dedupe_level1 = os.environ.get('KGE_TRANSE_DEDUPE_L1', '0') == '1'
    # the count sweep is enqueued in front of the second stream's filter correction (evaluation.COUNT_FIRST: -3 % here)
    lp_count_first = True

    def _tables(self):
        return [self.ent_emb.weight, self.rel_emb.weight]

    def _abs_bounds(self):
        """Device scalars (max |E|, max |R|) of this evaluation (guard slots 3 / 4, cached per session): every query
        element of TransE is e +- r, so their sum bounds both operands of the L1 prefilter."""
        emax, rmax = guard_slot(self._lp_guard, G_XABS), guard_slot(self._lp_guard, G_YABS)
        E, R = _hip.f32c(self.ent_emb.weight.data), _hip.f32c(self.rel_emb.weight.data)
        self._cache.get('sad_emax', [E], lambda: _hip.absmax(E, emax))
        self._cache.get('sad_rmax', [R], lambda: _hip.absmax(R, rmax))
        return emax, rmax

    def _hip_kind(self):
        return _hip.TRANSE_L1 if self.dissimilarity_type == 'L1' else _hip.TRANSE_L2

    def normalize_parameters(self):
        """L2-normalise entity embeddings (translation.py:83-90)."""
        self._normalize_weight_(self.ent_emb)

    def get_embeddings(self):
        self.normalize_parameters()
        return self.ent_emb.weight.data, self.rel_emb.weight.data

    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """(h, t, r, candidates); candidates is a stride-0 (b, N, d) view of the
        table, as in the reference (translation.py:105-125)."""
        self._check_unsharded('inference_prepare_candidates')
        b_size = max(h_idx.shape[0], t_idx.shape[0], r_idx.shape[0])   # inference passes one empty index
        E, R = self.ent_emb.weight.data, self.rel_emb.weight.data
        h, t, r = _hip.gather_rows(E, h_idx), _hip.gather_rows(E, t_idx), _hip.gather_rows(R, r_idx)
        if entities:
            candidates = E.view(1, self.n_ent, self.emb_dim).expand(b_size, self.n_ent, self.emb_dim)
        else:
            candidates = R.view(1, self.n_rel, self.emb_dim).expand(b_size, self.n_rel, self.emb_dim)
        return h, t, r, candidates

    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        tabs = [x.data for x in self._tables()]
        sd = _hip.side_code(side)
        fusable = (self.dissimilarity_type == 'L2' and self.l2_mode == 'auto' and self._guard_on and self._expand_ok is None
                   and self.split_filter and self._split_ok and h_idx.shape[0] > 0 and self.emb_dim % 4 == 0)
        if fusable and ent_lo == 0 and ent_hi == self.n_ent and self._row_shard is None:
            return self._fused_query_problem(h_idx, t_idx, r_idx, sd, tabs, cols if sd == _hip.SIDE_BOTH else None)
        if fusable and qtabs is not None and self._row_shard == (ent_lo, ent_hi) and sd == _hip.SIDE_BOTH:
            # ROW-SHARDED table with the replicas of the query entities' rows at hand (h_idx / t_idx index THEM): the same
            # fused query side, fed from the replicas; candidates = this rank's rows
            return self._fused_query_problem(h_idx, t_idx, r_idx, sd, tabs, None, qrep=_hip.f32c(qtabs[0]), c_base=ent_lo)
        Q0, _, _, _ = self._lp_prep(sd, h_idx, t_idx, r_idx, exchange, qtabs=qtabs)
        prob = self._translational_problem(Q0, self._cand_rows(_hip.f32c(tabs[0]), ent_lo, ent_hi),
                                           c_base=ent_lo)
        # (L2: f16-split count over columns; L1: the SAD count; broadcast-subtract L2: the packed-FMA count)
        plain_l2_direct = int(prob.desc.mode) == _hip.LP_L2_DIRECT and not prob.desc.Wq    # (kge_lp_count_ge_cols)
        prob.cols = cols if (sd == _hip.SIDE_BOTH and (prob.split is not None or prob.sad is not None or plain_l2_direct)) \
            else None
        return prob

    def _fused_query_problem(self, h_idx, t_idx, r_idx, sd, tabs, cols=None, qrep=None, c_base=0):
        """Inside evaluate(): the whole query side of a batch (q, ||q||^2, true scores, split queries, thresholds) from
        ONE kernel; the evaluator's pair_scores(true_idx) / count_ge calls then find their inputs ready.
        ``qrep`` (row-sharded tables, r05): replicas of the rows of the entities the queries mention -- the source and
        true-entity rows are read from THEM (h_idx / t_idx index the replicas; same rows, same chains, same bits as the
        owner shard's), while the candidate side -- norms, split / hi table, the bounds of the error band -- is this
        rank's own rows ``tabs[0]`` = global entities [c_base, c_base + rows)."""
        E = _hip.f32c(tabs[0])
        key = (c_base, E.shape[0])
        Eq = E if qrep is None else qrep            # where the query pipeline reads e_src / e_true
        level = self._level_and_frag()
        lvl1, frag = level                          # (r06: grouped columns run on the free-running kernel too)
        # the candidate side: on the free-running sweep ONE launch; every query pipeline launch folds its block maxima
        prep, en = self._cand_norms(key, E, None, frag)
        split = self._split_operand(key, E, aug=en, level=level, prep=prep)

        def enq():      # ||.||^2 of the rows the true scores are read from (replicas: their own chain norms, no maximum)
            if qrep is None:
                return en
            return self._cache.get('en_replica', [qrep], lambda: _hip.row_sqnorm(qrep))
        emax, qmax = guard_slot(self._lp_guard, G_EMAX), guard_slot(self._lp_guard, G_QMAX)
        if lvl1:
            pre = _hip.lp_query_pipeline(sd, Eq, tabs[1], h_idx, t_idx, r_idx, enq(), emax, qmax, cols=cols, level=1,
                                         de2max=split['de2max'], tp_bmax=prep[2] if prep is not None else None,
                                         zero_counts=True, regions=bool(frag) and bool(getattr(self, '_lp_regions', False)))
        else:
            pre = _hip.lp_query_pipeline(sd, Eq, tabs[1], h_idx, t_idx, r_idx, enq(), emax, qmax, e2pref=split['e2pref'],
                                         cols=cols, zero_counts=True)
        # (SIDE_BOTH: the evaluator fills in the concatenated true indices it gets from the filter lookup)
        pre['true_idx'] = t_idx if sd == _hip.SIDE_TAIL else (h_idx if sd == _hip.SIDE_HEAD else None)
        prob = _hip.LpProblem(_hip.LP_L2_EXPAND, pre['Q'], E, qn=pre['qn'], en=en, c_base=c_base)
        prob.split = split
        prob.pre = pre
        return prob


class TorusEModel(TranslationModel):
    """TorusE (translation.py:655-767).  ``TorusEModel(emb_dim, n_entities, n_relations, dissimilarity_type)`` with type
    'L1', 'torus_L1', 'torus_L2' or 'torus_eL2'; parameters ``ent_emb``, ``rel_emb``.

    Embeddings live in (-1, 1) -- ``normalize_parameters`` is ``frac_`` (x - trunc(x), the sign kept).  The torus
    dissimilarities have no GEMM form: every all-candidates problem is a broadcast-subtract one on the VALU
    (KGE_LP_TORUS_L1 / _L2 / _EL2; 'L1' is KGE_LP_L1_DIRECT), and the reference's (b, N, d) candidate broadcast is never
    built.  Relation prediction scores -diss(h + r_c, t) over the relation table (the reference raises AttributeError
    there, translation.py:765)."""

    _ENT_TABLES = ('ent_emb',)
    _SCORE_KIND = {'L1': _hip.TORUSE_L1, 'torus_L1': _hip.TORUSE_TORUS_L1, 'torus_L2': _hip.TORUSE_TORUS_L2,
                   'torus_eL2': _hip.TORUSE_TORUS_EL2}

    def __init__(self, emb_dim, n_entities, n_relations, dissimilarity_type):
        assert dissimilarity_type in ['L1', 'torus_L1', 'torus_L2', 'torus_eL2']
        super().__init__(n_entities, n_relations, dissimilarity_type)
        self.emb_dim = emb_dim
        self.ent_emb = init_embedding(self.n_ent, self.emb_dim)
        self.rel_emb = init_embedding(self.n_rel, self.emb_dim)
        self.normalized = False
        # translation.py:701-702: normalize_parameters() on the freshly initialised (host) tables
        self.ent_emb.weight.data.frac_()
        self.rel_emb.weight.data.frac_()
        self.normalized = True

    def _tables(self):
        return [self.ent_emb.weight, self.rel_emb.weight]

    def _hip_kind(self):
        # the query rows of every all-candidates problem are TransE's: E[h] + R[r] | E[t] - R[r] (kge_lp_prep)
        return _hip.TRANSE_L1

    def scoring_function(self, h_idx, t_idx, r_idx):
        """-diss(frac(h) + frac(r), frac(t)) of the gathered rows (translation.py:705-721), one fused HIP kernel; the
        tables are not changed, and autograd sees frac as the identity (the reference applies it to ``.data``)."""
        object.__setattr__(self, 'normalized', False)
        self._check_unsharded('scoring_function')
        tables = self._tables()
        _hip.require_cuda(h_idx, t_idx, r_idx, *tables)
        return _ScoreTriples.apply(self._SCORE_KIND[self.dissimilarity_type], self.emb_dim, self.emb_dim, h_idx, t_idx,
                                   r_idx, *tables)

    def _triple_kind(self):
        return self._SCORE_KIND[self.dissimilarity_type]

    def forward_grouped(self, *args, **kwargs):
        """``Model.forward_grouped``; as ``scoring_function`` it marks the tables as no longer normalised."""
        object.__setattr__(self, 'normalized', False)
        return super().forward_grouped(*args, **kwargs)

    def normalize_parameters(self):
        """Project the embeddings on the torus: frac_ of both tables in place (translation.py:723-728, kge_frac_rows)."""
        for emb in (self.ent_emb, self.rel_emb):
            w = emb.weight.data
            _hip.require_cuda(w)
            if not w.is_contiguous():
                w = w.contiguous()
                emb.weight.data = w
            _hip.frac_rows_(w)
        object.__setattr__(self, 'normalized', True)

    def lp_eval_prepare(self):
        """The reference's evaluation calls inference_prepare_candidates, which frac's the tables when
        scoring_function ran since the last normalisation (translation.py:752-753)."""
        if not self.normalized:
            self.normalize_parameters()

    def get_embeddings(self):
        self.normalize_parameters()
        return self.ent_emb.weight.data, self.rel_emb.weight.data

    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """(h, t, r, candidates) (translation.py:742-767), after the in-place frac if the tables are not normalized.
        Entity candidates are an EntityCandidates handle, not a (b, N, d) tensor; relation candidates are the
        stride-0 (b, n_rel, d) view of the relation table."""
        self._check_unsharded('inference_prepare_candidates')
        if not self.normalized:
            self.normalize_parameters()
        b_size = max(h_idx.shape[0], t_idx.shape[0], r_idx.shape[0])   # inference passes one empty index
        E, R = self.ent_emb.weight.data, self.rel_emb.weight.data
        h, t, r = _hip.gather_rows(E, h_idx), _hip.gather_rows(E, t_idx), _hip.gather_rows(R, r_idx)
        if entities:
            candidates = EntityCandidates(self, _hip.i64c(r_idx), b_size)
        else:
            candidates = R.view(1, self.n_rel, self.emb_dim).expand(b_size, self.n_rel, self.emb_dim)
        return h, t, r, candidates

    def _handle_problem(self, q, cand, ent_lo=0, ent_hi=None):
        ent_hi = self.n_ent if ent_hi is None else ent_hi
        E = _hip.f32c(self.ent_emb.weight.data)
        return self._translational_problem(q, self._cand_rows(E, ent_lo, ent_hi), c_base=ent_lo)

    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        """s[i, c] = -diss(q_i - e_c) with q = h + r (tail side) / t - r (head side) for the entities [ent_lo, ent_hi):
        one broadcast-subtract problem (row-sharded tables: ``exchange`` / ``qtabs`` as TransE)."""
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        tabs = [x.data for x in self._tables()]
        sd = _hip.side_code(side)
        Q0, _, _, _ = self._lp_prep(sd, h_idx, t_idx, r_idx, exchange, qtabs=qtabs)
        return self._translational_problem(Q0, self._cand_rows(_hip.f32c(tabs[0]), ent_lo, ent_hi), c_base=ent_lo)


def _both_r(r_idx, sd, hint=None):
    """Relation id per query: the 2B queries of a both-sides batch are the B facts twice (``hint``: that vector, precomputed by
    the evaluator with the batch's FilterPlan)."""
    r_idx = _hip.i64c(r_idx)
    if sd == _hip.SIDE_BOTH and hint is not None and hint.shape[0] == 2 * r_idx.shape[0] and hint.device == r_idx.device:
        return hint
    return torch.cat([r_idx, r_idx]) if sd == _hip.SIDE_BOTH else r_idx


class TransHModel(TranslationModel):
    """TransH (translation.py:128-284).  ``TransHModel(emb_dim, n_entities,
    n_relations)``; parameters ``ent_emb``, ``rel_emb``, ``norm_vect``."""

    def __init__(self, emb_dim, n_entities, n_relations):
        super().__init__(n_entities, n_relations, dissimilarity_type='L2')
        self.emb_dim = emb_dim
        self.ent_emb = init_embedding(self.n_ent, self.emb_dim)
        self.rel_emb = init_embedding(self.n_rel, self.emb_dim)
        self.norm_vect = init_embedding(self.n_rel, self.emb_dim)
        self._host_normalize()
        self.evaluated_projections = False

    _kind = _hip.TRANSH
    _ENT_TABLES = ('ent_emb',)
    # the count kernel's epilogue gathers X[r_i, c]: queries processed in relation order share those rows
    lp_sort_queries_by_relation = True
    lp_dedupe_queries = 'relation-major'   # ColumnPlan with the columns in relation order (same reason)
    lp_stream_columns = False              # (the free-running kernel's projection epilogue sweeps per query)
    _lp_proj_counts = True                 # (... and exists for rows of its resident panel only: Model._level1_stream)

    def _tables(self):
        return [self.ent_emb.weight, self.rel_emb.weight, self.norm_vect.weight]

    @staticmethod
    def project(ent, norm_vect):
        return ent - (ent * norm_vect).sum(dim=1).view(-1, 1) * norm_vect

    def _host_normalize(self):
        F = torch.nn.functional
        self.ent_emb.weight.data = F.normalize(self.ent_emb.weight.data, p=2, dim=1)
        self.norm_vect.weight.data = F.normalize(self.norm_vect.weight.data, p=2, dim=1)
        self.rel_emb.weight.data = self.project(self.rel_emb.weight.data, self.norm_vect.weight.data)

    def normalize_parameters(self):
        """Normalise entities and normal vectors, re-project relations onto
        their hyperplanes (translation.py:208-219)."""
        self._normalize_weight_(self.ent_emb)
        self._normalize_weight_(self.norm_vect)
        R, W = self.rel_emb.weight.data, self.norm_vect.weight.data
        a = _hip.row_dot(R, W)                                   # (R.W) per relation
        # r - (r.w) w   via the ewise kernel: a*w then r - that
        aw = _hip.ewise(_hip.EW_MUL, a.view(-1, 1).expand_as(W).contiguous(), W)
        self.rel_emb.weight.data = _hip.ewise(_hip.EW_SUB, R, aw)

    def get_embeddings(self):
        self.normalize_parameters()
        return self.ent_emb.weight.data, self.rel_emb.weight.data, self.norm_vect.weight.data

    def _a_matrix(self, lo, hi):
        """a[c, r] = E[c].W[r] for c in [lo, hi): the only thing the
        reference's projected_entities cache is needed for (translation.py:272-281)."""
        E, W = _hip.f32c(self.ent_emb.weight.data), _hip.f32c(self.norm_vect.weight.data)
        Es = self._cand_rows(E, lo, hi)
        return self._cache.get('transh_a_%d_%d' % (lo, hi), [E, W],
                               lambda: _hip.LpProblem(_hip.LP_DOT, Es, W).scores())

    def _proj_problem(self, q, table, Wq, r_idx, c_base, K0, qn, en):
        """-||u - (e_c - x w)||^2 with x = e_c.w_{r_i}, expanded around the GEMM term u.e_c
        (KGE_LP_L2_PROJH): X[r, c] = W[r].E[c] is one small GEMM per evaluation, the
        per-query scalars are p = 2 u.w and z = ||w||^2 - 2."""
        XT, _ = self._proj_side_tables(table, c_base, K0)
        pz = torch.stack([_hip.row_dot(q, Wq, scale=2.0), _hip.row_sqnorm(Wq) - 2.0], dim=1).contiguous()
        prob = _hip.LpProblem(_hip.LP_L2_PROJH, q, table, qn=qn, en=en, Wq=pz, scal=XT, r_idx=r_idx,
                              c_base=c_base)
        return self._attach_proj_split(prob, table, en, XT, None, K0)

    def _proj_side_tables(self, table, c_base, K0):
        """(X, None): X[r, c] = W[r].E[c] for the candidate rows, one small GEMM per evaluation."""
        W = _hip.f32c(self.norm_vect.weight.data)
        n = table.shape[0]

        def build():    # (n_rel, n) view of a row-padded buffer: the split kernel reads whole 256-candidate tiles
            # (only the padding columns need the zeros -- the GEMM writes the rest: a strided fill of < 256 columns instead of
            # one of the whole 13.8 MB buffer)
            buf = torch.empty(W.shape[0], _hip.padded_cols(n), dtype=torch.float32, device=table.device)
            if buf.shape[1] > n:
                buf[:, n:].zero_()
            return _hip.LpProblem(_hip.LP_DOT, W, table).scores(buf[:, :n])
        return self._cache.get('transh_aT_%d_%d' % (c_base, n), [table, W], build), None

    def evaluate_projections(self):
        """Kept for API compatibility (translation.py:260-284); the engine needs
        no (n_rel, n_ent, d) cache, so this only marks the projections valid."""
        self.evaluated_projections = True

    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """(proj_h, proj_t, r, candidates) (translation.py:234-258); candidates
        is an EntityCandidates handle, not a (b, N, d) copy."""
        self._check_unsharded('inference_prepare_candidates')
        tabs = [x.data for x in self._tables()]
        d = self.emb_dim
        if not entities:    # translation.py:252-256: every entity projected under EVERY relation
            r = _hip.gather_rows(tabs[1], r_idx)
            cand = tabs[1].view(1, self.n_rel, d).expand(h_idx.shape[0], self.n_rel, d)
            return (RelationProjections(self, _hip.i64c(h_idx), _hip.SIDE_PROJ_H),
                    RelationProjections(self, _hip.i64c(t_idx), _hip.SIDE_PROJ_T), r, cand)
        proj_h, proj_t = _projections(_hip.TRANSH, tabs, d, d, h_idx, t_idx, r_idx)
        r = _hip.gather_rows(tabs[1], r_idx)
        return proj_h, proj_t, r, EntityCandidates(self, _hip.i64c(r_idx), max(h_idx.shape[0], t_idx.shape[0]))

    def _relation_scores_proj(self, proj_h, proj_t, r):
        R = self.rel_emb.weight.data
        tab = _table_of(r)
        if tab is None or tab.data_ptr() != R.data_ptr() or tab.shape != R.shape:
            return None
        return _hip.relation_scores_proj(_hip.TRANSH, self.ent_emb.weight.data, R, self.norm_vect.weight.data, None,
                                         self.emb_dim, self.emb_dim, proj_h.idx, proj_t.idx)

    def _handle_problem(self, q, cand, ent_lo=0, ent_hi=None):
        ent_hi = self.n_ent if ent_hi is None else ent_hi
        E, W = _hip.f32c(self.ent_emb.weight.data), self.norm_vect.weight.data
        Wq = _hip.gather_rows(W, cand.r_idx)
        return self._translational_problem(q, self._cand_rows(E, ent_lo, ent_hi), Wq=Wq,
                                           scal=lambda: self._a_matrix(ent_lo, ent_hi), r_idx=cand.r_idx,
                                           c_base=ent_lo)

    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        tabs = [x.data for x in self._tables()]
        sd = _hip.side_code(side)
        r_both = _both_r(r_idx, sd, getattr(self, '_lp_r_both', None))
        if self._proj_fast_ok() and h_idx.shape[0] > 0:
            W = _hip.f32c(self.norm_vect.weight.data)
            prob = self._proj_fast_problem(sd, h_idx, t_idx, r_idx, r_both, ent_lo, ent_hi, exchange, qtabs,
                                           (_hip.LP_L2_PROJH, W, 2.0, -2.0, None, self._proj_side_tables))
            if prob is not None:
                prob.cols = cols if (sd == _hip.SIDE_BOTH and prob.split is not None) else None
                return prob
        Q0, _, _, Wq = self._lp_prep(sd, h_idx, t_idx, r_idx, exchange, qtabs=qtabs, want_w=True)
        prob = self._translational_problem(Q0, self._cand_rows(_hip.f32c(tabs[0]), ent_lo, ent_hi), Wq=Wq,
                                           scal=lambda: self._a_matrix(ent_lo, ent_hi),
                                           r_idx=r_both, c_base=ent_lo)
        prob.cols = cols if (sd == _hip.SIDE_BOTH and prob.split is not None) else None
        return prob


class TransDModel(TranslationModel):
    """TransD (translation.py:461-652).  ``TransDModel(ent_emb_dim, rel_emb_dim,
    n_entities, n_relations)``; parameters ``ent_emb``, ``rel_emb``,
    ``ent_proj_vect``, ``rel_proj_vect``.  Needs ent_emb_dim >= rel_emb_dim
    (the reference's ``ent[:, :rel_emb_dim]`` slice, :568)."""

    _kind = _hip.TRANSD
    _ENT_TABLES = ('ent_emb', 'ent_proj_vect')
    _ENT_POS = (0, 2)
    lp_sort_queries_by_relation = True     # (as TransH: the epilogue gathers G[r_i, c])
    lp_dedupe_queries = 'relation-major'
    lp_stream_columns = False
    _lp_proj_counts = True

    def __init__(self, ent_emb_dim, rel_emb_dim, n_entities, n_relations):
        super().__init__(n_entities, n_relations, 'L2')
        self.ent_emb_dim = ent_emb_dim
        self.rel_emb_dim = rel_emb_dim
        self.ent_emb = init_embedding(self.n_ent, self.ent_emb_dim)
        self.rel_emb = init_embedding(self.n_rel, self.rel_emb_dim)
        self.ent_proj_vect = init_embedding(self.n_ent, self.ent_emb_dim)
        self.rel_proj_vect = init_embedding(self.n_rel, self.rel_emb_dim)
        F = torch.nn.functional
        for emb in (self.ent_emb, self.rel_emb, self.ent_proj_vect, self.rel_proj_vect):
            emb.weight.data = F.normalize(emb.weight.data, p=2, dim=1)
        self.evaluated_projections = False

    def _tables(self):
        return [self.ent_emb.weight, self.rel_emb.weight, self.ent_proj_vect.weight,
                self.rel_proj_vect.weight]

    def normalize_parameters(self):
        """L2-normalise all four tables (translation.py:570-579)."""
        for emb in (self.ent_emb, self.rel_emb, self.ent_proj_vect, self.rel_proj_vect):
            self._normalize_weight_(emb)

    def get_embeddings(self):
        self.normalize_parameters()
        return (self.ent_emb.weight.data, self.rel_emb.weight.data,
                self.ent_proj_vect.weight.data, self.rel_proj_vect.weight.data)

    def _neg_sigma(self, lo, hi):
        """-s[c], s[c] = Ep[c].E[c]: all the reference's projected_entities
        cache depends on per entity (translation.py:641-646)."""
        E, Ep = _hip.f32c(self.ent_emb.weight.data), _hip.f32c(self.ent_proj_vect.weight.data)
        return self._cache.get('transd_s_%d_%d' % (lo, hi), [E, Ep],
                               lambda: _hip.row_dot(self._cand_rows(Ep, lo, hi), self._cand_rows(E, lo, hi), scale=-1.0))

    def evaluate_projectionss(self):
        """Kept for API compatibility (translation.py:629-652, reference spelling)."""
        self.evaluated_projections = True

    evaluate_projections = evaluate_projectionss

    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """(proj_h, proj_t, r, candidates) (translation.py:603-627)."""
        self._check_unsharded('inference_prepare_candidates')
        tabs = [x.data for x in self._tables()]
        de, dr = self.ent_emb_dim, self.rel_emb_dim
        if not entities:    # translation.py:621-626
            r = _hip.gather_rows(tabs[1], r_idx)
            cand = tabs[1].view(1, self.n_rel, dr).expand(h_idx.shape[0], self.n_rel, dr)
            return (RelationProjections(self, _hip.i64c(h_idx), _hip.SIDE_PROJ_H),
                    RelationProjections(self, _hip.i64c(t_idx), _hip.SIDE_PROJ_T), r, cand)
        proj_h, proj_t = _projections(_hip.TRANSD, tabs, de, dr, h_idx, t_idx, r_idx)
        r = _hip.gather_rows(tabs[1], r_idx)
        return proj_h, proj_t, r, EntityCandidates(self, _hip.i64c(r_idx), max(h_idx.shape[0], t_idx.shape[0]))

    def _relation_scores_proj(self, proj_h, proj_t, r):
        R = self.rel_emb.weight.data
        tab = _table_of(r)
        if tab is None or tab.data_ptr() != R.data_ptr() or tab.shape != R.shape:
            return None
        return _hip.relation_scores_proj(_hip.TRANSD, self.ent_emb.weight.data, R, self.rel_proj_vect.weight.data,
                                         self.ent_proj_vect.weight.data, self.ent_emb_dim, self.rel_emb_dim,
                                         proj_h.idx, proj_t.idx)

    def _problem(self, q, Wq, ent_lo, ent_hi, r_idx=None):
        E = _hip.f32c(self.ent_emb.weight.data)
        # candidates use E[c, :d_r]: same rows, inner dim K0 = d_r, leading dim d_e
        return self._translational_problem(q, self._cand_rows(E, ent_lo, ent_hi), Wq=Wq,
                                           scal=lambda: self._neg_sigma(ent_lo, ent_hi), c_base=ent_lo,
                                           K0=self.rel_emb_dim, r_idx=r_idx)

    def _proj_problem(self, q, table, Wq, r_idx, c_base, K0, qn, en):
        """-||u - (e'_c + y_c w)||^2, e' = e[:d_r], y_c = ep_c.e_c, expanded around the GEMM
        term u.e'_c (KGE_LP_L2_PROJD): G[r, c] = Rp[r].e'_c is one small GEMM per evaluation,
        the per-query scalars are p = -2 u.w and z = ||w||^2."""
        GT, sigma = self._proj_side_tables(table, c_base, K0)
        pz = torch.stack([_hip.row_dot(q, Wq, scale=-2.0), _hip.row_sqnorm(Wq)], dim=1).contiguous()
        prob = _hip.LpProblem(_hip.LP_L2_PROJD, q, table, qn=qn, en=en, Wq=pz, scal=GT, r_idx=r_idx, yc=sigma,
                              c_base=c_base, K0=K0)
        return self._attach_proj_split(prob, table, en, GT, sigma, K0)

    def _proj_side_tables(self, table, c_base, K0):
        """(G, sigma): G[r, c] = Rp[r].E[c, :d_r] (one small GEMM per evaluation) and sigma[c] = Ep[c].E[c]."""
        lo, hi = c_base, c_base + table.shape[0]
        Rp = _hip.f32c(self.rel_proj_vect.weight.data)
        Ep = _hip.f32c(self.ent_proj_vect.weight.data)
        n = table.shape[0]

        def build_g():
            buf = torch.empty(Rp.shape[0], _hip.padded_cols(n), dtype=torch.float32, device=table.device)
            if buf.shape[1] > n:
                buf[:, n:].zero_()
            return _hip.LpProblem(_hip.LP_DOT, Rp, table, K0=K0).scores(buf[:, :n])

        def build_s():
            buf = torch.zeros(_hip.padded_cols(n), dtype=torch.float32, device=table.device)
            buf[:n] = _hip.row_dot(self._cand_rows(Ep, lo, hi), table, scale=1.0)
            return buf[:n]
        GT = self._cache.get('transd_gT_%d_%d' % (lo, hi), [table, Rp], build_g)
        sigma = self._cache.get('transd_sp_%d_%d' % (lo, hi), [table, Ep], build_s)
        return GT, sigma

    def _handle_problem(self, q, cand, ent_lo=0, ent_hi=None):
        ent_hi = self.n_ent if ent_hi is None else ent_hi
        Wq = _hip.gather_rows(self.rel_proj_vect.weight.data, cand.r_idx)
        return self._problem(q, Wq, ent_lo, ent_hi, r_idx=cand.r_idx)

    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        sd = _hip.side_code(side)
        r_both = _both_r(r_idx, sd, getattr(self, '_lp_r_both', None))
        if self._proj_fast_ok() and h_idx.shape[0] > 0:
            Rp = _hip.f32c(self.rel_proj_vect.weight.data)
            prob = self._proj_fast_problem(sd, h_idx, t_idx, r_idx, r_both, ent_lo, ent_hi, exchange, qtabs,
                                           (_hip.LP_L2_PROJD, Rp, -2.0, 0.0, self.rel_emb_dim, self._proj_side_tables))
            if prob is not None:
                prob.cols = cols if (sd == _hip.SIDE_BOTH and prob.split is not None) else None
                return prob
        Q0, _, _, Wq = self._lp_prep(sd, h_idx, t_idx, r_idx, exchange, qtabs=qtabs, want_w=True)
        prob = self._problem(Q0, Wq, ent_lo, ent_hi, r_idx=r_both)
        prob.cols = cols if (sd == _hip.SIDE_BOTH and prob.split is not None) else None
        return prob


class _RelationGroupedProblem(object):
    """TransR's exact all-candidates problem: for every relation rho among the queries, P_rho = E M_rho^T (one KGE_LP_DOT
    problem, (N, d_r)) and then KGE_LP_L2_DIRECT of rho's queries against P_rho -- the reference's
    -||q - M_rho e_c||^2 without any cancellation.  One P_rho exists at a time; nothing of (n_rel, N, d_r) is kept.  It
    answers what the evaluators ask of an LpProblem.  Building it reads the batch's relations on the host (one sync)."""

    split = sad = pre = cols = pre_q = zero_counts = None

    def __init__(self, Q, r_q, table, M, d_e, d_r, c_base):
        self.Q, self.table, self.c_base = Q, table, c_base
        self.M3 = M.view(M.shape[0], d_r, d_e)
        self.B, self.N, self.device = Q.shape[0], table.shape[0], Q.device
        if Q.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('torchkge_amd: TransR\'s exact relation-grouped path reads the batch\'s relations on the host '
                               'and cannot be captured into a graph: evaluate with graph=False when l2_mode is not \'auto\'')
        rels, inv = torch.unique(r_q, return_inverse=True)
        order = _hip.sort_perm(inv, max(int(rels.shape[0]), 1)) if Q.shape[0] else inv
        counts = torch.bincount(inv, minlength=rels.shape[0]).tolist()
        self.groups, lo = [], 0
        for rho, n in zip(rels.tolist(), counts):
            self.groups.append((rho, order[lo:lo + n]))
            lo += n

    def _each(self, q0=None, q1=None):
        """(query positions, KGE_LP_L2_DIRECT problem) per relation present; q0 / q1: only the queries of that range."""
        for rho, idx in self.groups:
            if q0 is not None:
                idx = idx[(idx >= q0) & (idx < q1)]
            if idx.shape[0] == 0 or self.N == 0:
                continue
            P = _hip.LpProblem(_hip.LP_DOT, self.table, _hip.f32c(self.M3[rho])).scores()
            yield idx, _hip.LpProblem(_hip.LP_L2_DIRECT, _hip.gather_rows(self.Q, idx), P, c_base=self.c_base)

    def scores(self, out=None):
        if out is None:
            out = torch.empty(self.B, self.N, dtype=torch.float32, device=self.device)
        for idx, prob in self._each():
            out[idx] = prob.scores()
        return out

    def scores_chunk(self, c0, c1, out):
        for idx, prob in self._each():
            tmp = torch.empty(idx.shape[0], c1 - c0, dtype=torch.float32, device=self.device)
            out[idx, :c1 - c0] = prob.scores_chunk(c0, c1, tmp)
        return out

    def scores_rows(self, q0, q1, out):
        for idx, prob in self._each(q0, q1):
            out[idx - q0, :self.N] = prob.scores()
        return out

    def pair_scores(self, ci, qi=None):
        ci = _hip.i64c(ci)
        out = torch.zeros(ci.shape[0], dtype=torch.float32, device=self.device)
        if qi is None:
            for idx, prob in self._each():
                out[idx] = prob.pair_scores(ci[idx])
            return out
        qi = _hip.i64c(qi)
        pos_of = torch.empty(self.B, dtype=torch.int64, device=self.device)
        for idx, prob in self._each():      # the pairs whose query belongs to this relation, re-indexed into its sub-problem
            member = torch.zeros(self.B, dtype=torch.bool, device=self.device)
            member[idx] = True
            pos_of[idx] = torch.arange(idx.shape[0], device=self.device)
            sel = member[qi].nonzero().view(-1)
            if sel.shape[0]:
                out[sel] = prob.pair_scores(ci[sel], pos_of[qi[sel]])
        return out

    def count_ge(self, s_true, raw=None):
        if raw is None:
            raw = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        for idx, prob in self._each():
            raw[idx] += prob.count_ge(s_true[idx].contiguous())
        return raw

    def filter_sub(self, s_true, true_idx, seg_lo, seg_hi, targets, sub=None, found=None, grouped=False, plan=None):
        if sub is None:
            sub = torch.empty(self.B, dtype=torch.int32, device=self.device)
        if found is None:
            found = torch.empty(self.B, dtype=torch.int32, device=self.device)
        for idx, prob in self._each():
            s, f = prob.filter_sub(s_true[idx].contiguous(), true_idx[idx].contiguous(), seg_lo[idx].contiguous(),
                                   seg_hi[idx].contiguous(), targets)
            sub[idx] = s
            found[idx] = f
        return sub, found


class TransRModel(TranslationModel):
    """TransR (translation.py:287-458).  ``TransRModel(ent_emb_dim, rel_emb_dim, n_entities, n_relations)``; parameters
    ``ent_emb``, ``rel_emb``, ``proj_mat`` (n_rel, rel_emb_dim * ent_emb_dim).

    The reference's (n_rel, n_ent, rel_emb_dim) ``projected_entities`` cache is never built: with q = M_r e +- r and
    u = M_r^T q,  ||q - M_r e_c||^2 = ||q||^2 - 2 u.e_c + Z[r, c]  and  Z[r, c] = ||M_r e_c||^2  is one float per
    (relation, entity) (kge_transr_proj_sqnorm) -- a KGE_LP_L2_PROJH problem against the RAW entity table.  The rank counts
    run on the fp32 MFMA path: the f16 split prefilter is not attached (``prob.split`` stays None), because its certified
    band bounds |A0.T0| by sqrt(qn) max||e||, which does not hold for A0 = u.  Beyond ``L2_EXPAND_LIMIT`` (measured on
    max ||q||^2 + max Z) the exact relation-grouped path takes over (_RelationGroupedProblem); ``lp_last_path`` names
    the path the last problem took ('expand' or 'exact')."""

    _kind = _hip.TRANSR
    _DENSE_GRAD_TABLES = ('proj_mat',)      # reduced per relation by kge_transr_rel_grad: not row-shaped
    _ENT_TABLES = ('ent_emb',)
    lp_sort_queries_by_relation = True     # (the epilogue gathers Z[r_i, c]: queries in relation order share those rows)
    lp_last_path = None

    def __init__(self, ent_emb_dim, rel_emb_dim, n_entities, n_relations):
        super().__init__(n_entities, n_relations, 'L2')
        self.ent_emb_dim = ent_emb_dim
        self.rel_emb_dim = rel_emb_dim
        self.ent_emb = init_embedding(self.n_ent, self.ent_emb_dim)
        self.rel_emb = init_embedding(self.n_rel, self.rel_emb_dim)
        self.proj_mat = init_embedding(self.n_rel, self.rel_emb_dim * self.ent_emb_dim)
        F = torch.nn.functional     # translation.py:343: normalize_parameters() on the freshly initialised (host) tables
        self.ent_emb.weight.data = F.normalize(self.ent_emb.weight.data, p=2, dim=1)
        self.rel_emb.weight.data = F.normalize(self.rel_emb.weight.data, p=2, dim=1)
        self.evaluated_projections = False

    def _tables(self):
        return [self.ent_emb.weight, self.rel_emb.weight, self.proj_mat.weight]

    def scoring_function(self, h_idx, t_idx, r_idx):
        """-||M_r h^ + r - M_r t^||^2 (translation.py:345-366), one fused HIP kernel; as in the reference a call marks
        the projections stale."""
        object.__setattr__(self, 'evaluated_projections', False)
        return super().scoring_function(h_idx, t_idx, r_idx)

    def project(self, ent, proj_mat):
        """M e for (b, d_e) rows and (b, d_r, d_e) operators (translation.py:368-370; not on the engine's paths)."""
        return torch.matmul(proj_mat, ent.view(-1, self.ent_emb_dim, 1)).view(-1, self.rel_emb_dim)

    def normalize_parameters(self):
        """L2-normalise entity and relation embeddings; proj_mat is left alone (translation.py:372-381)."""
        self._normalize_weight_(self.ent_emb)
        self._normalize_weight_(self.rel_emb)

    def get_embeddings(self):
        self.normalize_parameters()
        return (self.ent_emb.weight.data, self.rel_emb.weight.data,
                self.proj_mat.weight.data.view(-1, self.rel_emb_dim, self.ent_emb_dim))

    def evaluate_projectionss(self):
        """Kept for API compatibility (translation.py:432-458, reference spelling): there is no cache to fill."""
        self.evaluated_projections = True

    def lp_true_scores_replica(self, prob, qctx):
        return None     # (the Z row of a true entity belongs to its owner shard: the owner's score, summed over the ranks)

    # ---- candidate side --------------------------------------------------------------------------------------------
    def _z_table(self, table, c_base, guard_max=None):
        """Z[r, c] = ||M_r e_c||^2 for the candidate rows, an (n_rel, n) view of a buffer padded as the projection modes
        want it; per evaluation.  ``guard_max``: its maximum is folded into that device scalar."""
        M = _hip.f32c(self.proj_mat.weight.data)
        n = table.shape[0]

        def build():
            buf = torch.empty(self.n_rel, _hip.padded_cols(n), dtype=torch.float32, device=table.device)
            if buf.shape[1] > n:
                buf[:, n:].zero_()
            _hip.transr_proj_sqnorm(M, table, self.ent_emb_dim, self.rel_emb_dim, out=buf)
            return buf
        buf = self._cache.get('transr_z_%d_%d' % (c_base, n), [table, M], build)
        if guard_max is not None:
            self._cache.get('transr_zmax_%d_%d' % (c_base, n), [buf], lambda: _hip.absmax(buf, guard_max))
        return buf[:, :n]

    def _problem(self, Q, U, r_q, table, c_base):
        """The all-candidates problem of the queries Q (rows, d_r) in relation space, U = M_r^T Q, relations r_q."""
        guarded = self.l2_mode == 'auto' and self._expand_ok is None and self._guard_on
        if self.l2_mode in ('expand', 'auto') and table.shape[0] > 0:
            gq, ge = (guard_slot(self._lp_guard, G_QMAX), guard_slot(self._lp_guard, G_EMAX)) if guarded else (None, None)
            qn = _hip.row_sqnorm(Q, max_io=gq)
            ok = True
            Z = None
            if self.l2_mode == 'auto' and not guarded:
                ok = self._expand_ok
                if ok is None:          # drop-in API call: decide now on the actual operands (one sync)
                    Z = self._z_table(table, c_base)
                    ok = Q.shape[0] == 0 or float((qn.max() + Z.max()).item()) <= self.L2_EXPAND_LIMIT
            if ok:
                if Z is None:
                    Z = self._z_table(table, c_base, ge)
                rows, n = Q.shape[0], table.shape[0]

                def ones_zeros():
                    pz = torch.zeros(rows, 2, dtype=torch.float32, device=Q.device)
                    pz[:, 0] = 1.0
                    return pz
                pz = self._cache.get('transr_pz_%d' % rows, [table], ones_zeros)
                en = self._cache.get('transr_en0_%d' % n, [table],
                                     lambda: torch.zeros(max(n, 1), dtype=torch.float32, device=Q.device))
                object.__setattr__(self, 'lp_last_path', 'expand')
                return _hip.LpProblem(_hip.LP_L2_PROJH, U, table, qn=qn, en=en, Wq=pz, scal=Z, r_idx=r_q, c_base=c_base)
        object.__setattr__(self, 'lp_last_path', 'exact')
        return _RelationGroupedProblem(Q, r_q, table, _hip.f32c(self.proj_mat.weight.data), self.ent_emb_dim,
                                       self.rel_emb_dim, c_base)

    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        E, R, M = [_hip.f32c(x.data) for x in self._tables()]
        sd = _hip.side_code(side)
        de, dr = self.ent_emb_dim, self.rel_emb_dim
        table = self._cand_rows(E, ent_lo, ent_hi)
        r_q = _both_r(r_idx, sd, getattr(self, '_lp_r_both', None))
        if qtabs is not None:               # replicas of the query entities' rows: h_idx / t_idx index them
            Q, U = _hip.transr_query(sd, _hip.f32c(qtabs[0]), M, R, de, dr, h_idx, t_idx, r_idx)
        elif self._row_shard is not None:   # the owner's rows, zero elsewhere, summed over the shards (x + 0 is exact)
            if exchange is None:
                raise RuntimeError('torchkge_amd: a row-sharded model needs the evaluator\'s query exchange')
            ids = torch.cat([h_idx, t_idx]) if sd == _hip.SIDE_BOTH else (h_idx if sd == _hip.SIDE_TAIL else t_idx)
            lo, hi = self._row_shard
            rows = _hip.lp_prep(_hip.TRANSE_L2, _hip.SIDE_PROJ_H, [E, E], de, de, ids, ids, torch.zeros_like(ids),
                                ent_lo=lo, ent_n=hi - lo)[0]
            exchange([rows])
            Q, U = _hip.transr_query(sd, rows, M, R, de, dr, None, None, r_idx)
        else:
            Q, U = _hip.transr_query(sd, E, M, R, de, dr, h_idx, t_idx, r_idx)
        return self._problem(Q, U, r_q, table, ent_lo)

    # ---- reference inference API -------------------------------------------------------------------------------------
    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """(proj_h, proj_t, r, candidates) (translation.py:405-430); entity candidates are an EntityCandidates handle,
        never a (b, N, d_r) copy; ``entities=False``: RelationProjections handles and the expanded relation table."""
        self._check_unsharded('inference_prepare_candidates')
        object.__setattr__(self, 'evaluated_projections', True)
        tabs = [x.data for x in self._tables()]
        de, dr = self.ent_emb_dim, self.rel_emb_dim
        r = _hip.gather_rows(tabs[1], r_idx)
        if not entities:
            cand = tabs[1].view(1, self.n_rel, dr).expand(h_idx.shape[0], self.n_rel, dr)
            return (RelationProjections(self, _hip.i64c(h_idx), _hip.SIDE_PROJ_H),
                    RelationProjections(self, _hip.i64c(t_idx), _hip.SIDE_PROJ_T), r, cand)
        proj_h, proj_t = _projections(_hip.TRANSR, tabs, de, dr, h_idx, t_idx, r_idx)
        return proj_h, proj_t, r, EntityCandidates(self, _hip.i64c(r_idx), max(h_idx.shape[0], t_idx.shape[0]))

    def _relation_scores_proj(self, proj_h, proj_t, r):
        R = self.rel_emb.weight.data
        tab = _table_of(r)
        if tab is None or tab.data_ptr() != R.data_ptr() or tab.shape != R.shape:
            return None
        E = self.ent_emb.weight.data
        X = _hip.ewise(_hip.EW_SUB, _hip.gather_rows(E, proj_h.idx), _hip.gather_rows(E, proj_t.idx))
        return _hip.transr_proj_sqnorm(self.proj_mat.weight.data, X, self.ent_emb_dim, self.rel_emb_dim, b=R,
                                       by_row=True).neg_()

    def _handle_problem(self, q, cand, ent_lo=0, ent_hi=None):
        ent_hi = self.n_ent if ent_hi is None else ent_hi
        E, _, M = [_hip.f32c(x.data) for x in self._tables()]
        q = _hip.f32c(q)
        _, U = _hip.transr_query(_hip.SIDE_TAIL, None, M, None, self.ent_emb_dim, self.rel_emb_dim, None, None,
                                 cand.r_idx, Q=q)
        return self._problem(q, U, cand.r_idx, self._cand_rows(E, ent_lo, ent_hi), ent_lo)


class RotatEModel(Model):
    """RotatE (Sun et al. 2019: "RotatE: Knowledge Graph Embedding by Relational Rotation in Complex Space"; not in the
    reference).  ``RotatEModel(emb_dim, n_entities, n_relations)``: entities are ``emb_dim`` complex numbers, a relation
    is a rotation by ``emb_dim`` phases, score = -sum_k |h_k r_k - t_k| with r_k = exp(i theta_k).

    Parameters: ``ent_emb`` (n_ent, 2 * emb_dim), a row stored INTERLEAVED as (re_0, im_0, re_1, im_1, ...) --
    ``torch.view_as_complex(weight.view(n_ent, emb_dim, 2))`` is its complex view -- and ``rel_emb`` (n_rel, emb_dim), the
    phases in radians, uniform in (-pi, pi).  No margin inside the score: gamma belongs to the criterion
    (``SelfAdversarialLoss(margin=...)``).

    Every all-candidates problem is the broadcast-subtract mode KGE_LP_CMOD of a query row q = h o r (tail side) or
    q = t o conj(r) (head side; |h r - t| = |h - t conj(r)| for a unit-modulus r) against the RAW entity table: the
    interleaved layout puts a complex coordinate inside the aligned group of four floats that the L1 / torus modes
    accumulate by, so nothing is repacked and no (b, N, 2d) tensor exists.  Relation prediction scores the b * n_rel
    expanded triples through the fused triple kernel."""

    _kind = _hip.ROTATE
    _ENT_TABLES = ('ent_emb',)
    MAX_EMB_DIM = 512       # kge_score_triples takes entity rows of at most 1024 floats, for every kind

    def __init__(self, emb_dim, n_entities, n_relations):
        if int(emb_dim) != emb_dim or not 1 <= emb_dim <= self.MAX_EMB_DIM:
            raise ValueError('torchkge_amd: RotatEModel needs 1 <= emb_dim <= %d (entity rows are 2 * emb_dim floats and the '
                             'fused triple kernels take rows of at most 1024), got %r' % (self.MAX_EMB_DIM, emb_dim))
        super().__init__(n_entities, n_relations)
        self.emb_dim = int(emb_dim)
        self.ent_emb = init_embedding(self.n_ent, 2 * self.emb_dim)
        self.rel_emb = init_embedding(self.n_rel, self.emb_dim)
        with torch.no_grad():
            self.rel_emb.weight.uniform_(-math.pi, math.pi)
        self.split_filter = False       # a modulus per coordinate has no GEMM form: no f16 prefilter, the exact VALU count

    def _tables(self):
        return [self.ent_emb.weight, self.rel_emb.weight]

    def _penalty_groups(self):
        """The complex modulus of every entity coordinate; no relation group: the phases parametrise unit-modulus
        numbers, there is nothing to shrink."""
        from .._hip_penalty import INTERLEAVED
        return [(INTERLEAVED, self.ent_emb.weight)], []

    def _uses_guard(self):
        return False

    def normalize_parameters(self):
        """Nothing to project: the phases are free and the entities unconstrained."""
        return None

    def get_embeddings(self):
        """(complex (n_ent, emb_dim) view of the entity table, (n_rel, emb_dim) phases)."""
        E = self.ent_emb.weight.data
        return torch.view_as_complex(E.contiguous().view(E.shape[0], self.emb_dim, 2)), self.rel_emb.weight.data

    # ---- all-candidates problems -----------------------------------------------------------------------------------
    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        """s[i, c] = -sum_k |q_ik - e_ck| (complex modulus) for the entities [ent_lo, ent_hi): ONE launch writes the query
        rows (kge_rotate_query), the candidates are the table's own rows.  Row-sharded tables: ``exchange`` / ``qtabs``
        as TransE."""
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        E, P = (_hip.f32c(x.data) for x in self._tables())
        sd = _hip.side_code(side)
        if qtabs is not None:       # replicas of the query entities' rows: h_idx / t_idx index THEM
            Q = _hip_rotate.rotate_query(sd, _hip.f32c(qtabs[0]), P, h_idx, t_idx, r_idx)
        elif self._row_shard is not None:
            if exchange is None:
                raise RuntimeError('torchkge_amd: a row-sharded model needs the evaluator\'s query exchange')
            Q = _hip_rotate.rotate_query(sd, E, P, h_idx, t_idx, r_idx, ent_lo=self._row_shard[0],
                                  ent_n=self._row_shard[1] - self._row_shard[0])
            exchange([Q])
        else:
            Q = _hip_rotate.rotate_query(sd, E, P, h_idx, t_idx, r_idx)
        return _hip.LpProblem(_hip.LP_CMOD, Q, self._cand_rows(E, ent_lo, ent_hi), c_base=ent_lo)

    # ---- reference inference API -----------------------------------------------------------------------------------
    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """(h, t, r, candidates): the gathered interleaved rows and phases; candidates is a stride-0 (b, N, 2 * emb_dim)
        view of the entity table, or with ``entities=False`` the (b, n_rel, emb_dim) one of the phase table."""
        self._check_unsharded('inference_prepare_candidates')
        b_size = max(h_idx.shape[0], t_idx.shape[0], r_idx.shape[0])   # inference passes one empty index
        E, P = self.ent_emb.weight.data, self.rel_emb.weight.data
        h, t, r = _hip.gather_rows(E, h_idx), _hip.gather_rows(E, t_idx), _hip.gather_rows(P, r_idx)
        if entities:
            candidates = E.view(1, self.n_ent, 2 * self.emb_dim).expand(b_size, self.n_ent, 2 * self.emb_dim)
        else:
            candidates = P.view(1, self.n_rel, self.emb_dim).expand(b_size, self.n_rel, self.emb_dim)
        return h, t, r, candidates

    RELATION_CHUNK = 1 << 20    # expanded triples per kge_score_triples launch of relation prediction

    def inference_scoring_function(self, h, t, r):
        """-sum_k |h_k r_k - t_k| against every candidate; the 3-D argument is the candidate set.  Entity candidates: the
        query rows of the gathered embeddings, then KGE_LP_CMOD.  Relation candidates: the b * n_rel triples (h_i, r_c,
        t_i), scored in chunks by the fused triple kernel on the gathered rows."""
        if torch.is_tensor(r) and r.dim() == 3:
            return self._relation_scores(h, t, r)
        assert r.dim() == 2
        tail = torch.is_tensor(t) and t.dim() == 3
        x, cand = (h, t) if tail else (t, h)
        assert torch.is_tensor(x) and x.dim() == 2 and torch.is_tensor(cand) and cand.dim() == 3
        _hip.require_cuda(x, r, cand)
        ids = torch.arange(x.shape[0], device=x.device)
        q = _hip_rotate.rotate_query(_hip.SIDE_TAIL if tail else _hip.SIDE_HEAD, x, r, ids, ids, ids)
        table = _table_of(cand)
        if table is not None:
            return _hip.LpProblem(_hip.LP_CMOD, q, _hip.f32c(table)).scores()
        return _hip.lp_scores_batched(_hip.LP_CMOD, q, cand)

    def _relation_scores(self, h, t, cand):
        _hip.require_cuda(h, t, cand)
        b, n_rel, d = cand.shape
        dev = h.device
        table = _table_of(cand)
        out = torch.empty(b, n_rel, dtype=torch.float32, device=dev)
        step = max(1, self.RELATION_CHUNK // max(n_rel, 1))
        rel = torch.arange(n_rel, device=dev)
        for b0 in range(0, b, step):
            n = min(step, b - b0)
            X = torch.cat([h[b0:b0 + n], t[b0:b0 + n]])             # entity rows of this chunk: heads, then tails
            hh = torch.arange(n, device=dev).repeat_interleave(n_rel)
            if table is not None:
                P, rr = _hip.f32c(table), rel.repeat(n)
            else:
                P, rr = cand[b0:b0 + n].reshape(n * n_rel, d), torch.arange(n * n_rel, device=dev)
            out[b0:b0 + n] = _hip.score_triples(_hip.ROTATE, [X, P], 2 * d, d, hh, hh + n, rr).view(n, n_rel)
        return out
