# -*- coding: utf-8 -*-
"""DistMult / ComplEx / RESCAL / HolE / ANALOGY with the reference's constructors, attributes
and state_dict keys (torchkge/models/bilinear.py:14-143, :146-267, :270-411,
:414-556, :559-763) on the HIP engine: the all-candidates score matrix is one fp32 MFMA
GEMM S = Q . E^T (ComplEx: K = 2d over the [Re | Im] tables, no concatenation;
RESCAL / HolE: Q = the relation-transformed query rows, kge_bilinear_query;
ANALOGY: K = scalar_dim + 2 complex_dim over the packed [sc | re | im] rows, kge_analogy_query)."""
import torch

from .. import _hip
from .. import _hip_analogy
from ..rowgrad import is_row_gradients
from ..utils.modeling import init_embedding
from ..utils.one_vs_all import one_vs_all_loss
from ..utils.k_vs_all import k_vs_all_loss
from .interfaces import BilinearModel, _table_of
from .translation import _ent_range


class DistMultModel(BilinearModel):
    """DistMult (bilinear.py:146-267): ``DistMultModel(emb_dim, n_entities,
    n_relations)``; parameters ``ent_emb`` (L2-normalised rows), ``rel_emb``."""

    _kind = _hip.DISTMULT
    _ENT_TABLES = ('ent_emb',)

    def __init__(self, emb_dim, n_entities, n_relations):
        super().__init__(emb_dim, n_entities, n_relations)
        self.ent_emb = init_embedding(self.n_ent, self.emb_dim)
        self.rel_emb = init_embedding(self.n_rel, self.emb_dim)
        self.ent_emb.weight.data = torch.nn.functional.normalize(self.ent_emb.weight.data, p=2, dim=1)

    def _tables(self):
        return [self.ent_emb.weight, self.rel_emb.weight]

    def normalize_parameters(self):
        """L2-normalise entity embeddings (bilinear.py:201-208)."""
        self._normalize_weight_(self.ent_emb)

    def get_embeddings(self):
        self.normalize_parameters()
        return self.ent_emb.weight.data, self.rel_emb.weight.data

    def inference_scoring_function(self, h, t, r):
        """Rank dispatch of bilinear.py:224-245: the 3-D argument is the
        candidate set; s = (a * b) . cand."""
        if t.dim() == 3:
            assert h.dim() == 2 and r.dim() == 2
            q, cand = _hip.ewise(_hip.EW_MUL, h, r), t          # tail completion
        elif h.dim() == 3:
            assert t.dim() == 2 and r.dim() == 2
            q, cand = _hip.ewise(_hip.EW_MUL, r, t), h          # head completion
        else:
            assert r.dim() == 3 and h.dim() == 2 and t.dim() == 2
            q, cand = _hip.ewise(_hip.EW_MUL, h, t), r          # relation prediction
        table = _table_of(cand)
        if table is not None:
            return _hip.LpProblem(_hip.LP_DOT, q, _hip.f32c(table)).scores()
        return _hip.lp_scores_batched(_hip.LP_DOT, q, cand)

    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """(h, t, r, candidates) with a stride-0 (b, N, d) candidates view
        (bilinear.py:247-267)."""
        self._check_unsharded('inference_prepare_candidates')
        b_size = max(h_idx.shape[0], t_idx.shape[0], r_idx.shape[0])   # inference passes one empty index
        E, R = self.ent_emb.weight.data, self.rel_emb.weight.data
        h, t, r = _hip.gather_rows(E, h_idx), _hip.gather_rows(E, t_idx), _hip.gather_rows(R, r_idx)
        if entities:
            candidates = E.view(1, self.n_ent, self.emb_dim).expand(b_size, self.n_ent, self.emb_dim)
        else:
            candidates = R.view(1, self.n_rel, self.emb_dim).expand(b_size, self.n_rel, self.emb_dim)
        return h, t, r, candidates

    def one_vs_all_loss(self, h_idx, t_idx, r_idx, side='both', label_smoothing=0.0, reduction='mean'):
        """Softmax cross-entropy of every fact's true tail among ALL entities as tails of (h, r, ?) (``side='tail'``),
        of its true head among all heads of (?, r, t) (``'head'``), or both as one problem of 2B queries, the tail side
        first like ``lp_problem_both`` (``'both'``).  ``label_smoothing`` and ``reduction`` as torch's ``cross_entropy``.

        The scores are those of ``inference_scoring_function`` on the RAW tables -- (e_h * r) . e_c -- exactly what the
        evaluator ranks.  The per-triple L2 normalisation of h and t inside ``scoring_function`` is NOT applied: keep the
        entity rows normalised with ``normalize_parameters()`` (OneVsAllTrainer does, per epoch).

        The (B, N) score matrix is never written (torchkge_amd.utils.one_vs_all).  The gradient of ``ent_emb`` is dense
        by nature -- every entity is a candidate of every query -- whatever ``row_gradients()`` says; so is
        ``rel_emb``'s here.  The query rows' part of it is summed by the ordered reduction under ``deterministic()``,
        the all-candidates part always in a fixed order."""
        return one_vs_all_loss(self, h_idx, t_idx, r_idx, side, label_smoothing, reduction)

    def k_vs_all_loss(self, ent_idx, r_idx, labels, side, label_smoothing=0.0, reduction='mean'):
        """Binary cross-entropy with logits of every key's scores over ALL entities against the set of its known
        answers: the keys are (h, r) = (``ent_idx``, ``r_idx``) scored against all tails (``side='tail'``) or (t, r)
        scored against all heads (``'head'``); ``labels = (seg_lo, seg_hi, targets)`` names each key's sorted answer
        list in place (``FilterIndex.lookup`` / ``.targets``).  ``reduction`` as torch's
        ``binary_cross_entropy_with_logits`` ('mean' divides by B * N); ``label_smoothing`` mixes every label with the
        uniform distribution over the entities (torchkge_amd.utils.k_vs_all).

        The scores are those of ``inference_scoring_function`` on the raw tables, exactly what the evaluator ranks, and
        neither the (B, N) score matrix nor a (B, N) label matrix is ever written.  The gradients of the tables are
        dense by nature; the query rows' part is summed by the ordered reduction under ``deterministic()``, the
        all-candidates part always in a fixed order."""
        return k_vs_all_loss(self, ent_idx, r_idx, labels, side, label_smoothing, reduction)

    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        tabs = [x.data for x in self._tables()]
        sd = _hip.side_code(side)
        if ent_lo == 0 and ent_hi == self.n_ent and self._row_shard is None and exchange is None and qtabs is None:
            prob = self._dot_fused_problem(sd, h_idx, t_idx, r_idx, [_hip.f32c(tabs[0])], [_hip.f32c(tabs[1])])
            if prob is not None:
                return prob
        Q0 = self._lp_prep(sd, h_idx, t_idx, r_idx, exchange, qtabs=qtabs)[0]
        T0 = self._cand_rows(_hip.f32c(tabs[0]), ent_lo, ent_hi)
        prob = self._attach_dot_split(_hip.LpProblem(_hip.LP_DOT, Q0, T0, c_base=ent_lo), T0, c_base=ent_lo)
        prob.cols = cols if (sd == _hip.SIDE_BOTH and prob.split is not None) else None
        return prob


class ComplExModel(BilinearModel):
    """ComplEx (bilinear.py:414-556): ``ComplExModel(emb_dim, n_entities,
    n_relations)``; parameters ``re_ent_emb``, ``im_ent_emb``, ``re_rel_emb``,
    ``im_rel_emb``; never normalised (:475-480)."""

    _kind = _hip.COMPLEX
    _ENT_TABLES = ('re_ent_emb', 'im_ent_emb')
    _ENT_POS = (0, 1)

    def __init__(self, emb_dim, n_entities, n_relations):
        super().__init__(emb_dim, n_entities, n_relations)
        self.re_ent_emb = init_embedding(self.n_ent, self.emb_dim)
        self.im_ent_emb = init_embedding(self.n_ent, self.emb_dim)
        self.re_rel_emb = init_embedding(self.n_rel, self.emb_dim)
        self.im_rel_emb = init_embedding(self.n_rel, self.emb_dim)

    def _tables(self):
        return [self.re_ent_emb.weight, self.im_ent_emb.weight, self.re_rel_emb.weight,
                self.im_rel_emb.weight]

    def _penalty_groups(self):
        """The complex modulus per coordinate of the entity pair and of the relation pair (Lacroix et al. 2018)."""
        from .._hip_penalty import SPLIT
        return ([(SPLIT, (self.re_ent_emb.weight, self.im_ent_emb.weight))],
                [(SPLIT, (self.re_rel_emb.weight, self.im_rel_emb.weight))])

    @property
    def _d_rel(self):
        return self.emb_dim

    def _lp_width(self):
        return 2 * self.emb_dim

    def normalize_parameters(self):
        """No normalisation for ComplEx (bilinear.py:475-480)."""
        pass

    def get_embeddings(self):
        return (self.re_ent_emb.weight.data, self.im_ent_emb.weight.data,
                self.re_rel_emb.weight.data, self.im_rel_emb.weight.data)

    def inference_scoring_function(self, h, t, r):
        """h, t, r are (re, im) tuples; the pair holding 3-D tensors is the
        candidate set (bilinear.py:501-528)."""
        re_h, im_h = h[0], h[1]
        re_t, im_t = t[0], t[1]
        re_r, im_r = r[0], r[1]
        E = _hip
        if re_t.dim() == 3:      # tail: (re_h re_r - im_h im_r).Re + (re_h im_r + im_h re_r).Im
            assert re_h.dim() == 2 and re_r.dim() == 2
            A = E.ewise(E.EW_MULSUB, re_h, re_r, im_h, im_r)
            Bq = E.ewise(E.EW_MULADD, re_h, im_r, im_h, re_r)
            cre, cim = re_t, im_t
        elif re_h.dim() == 3:    # head: Re.(re_r re_t + im_r im_t) + Im.(re_r im_t - im_r re_t)
            assert re_t.dim() == 2 and re_r.dim() == 2
            A = E.ewise(E.EW_MULADD, re_r, re_t, im_r, im_t)
            Bq = E.ewise(E.EW_MULSUB, re_r, im_t, im_r, re_t)
            cre, cim = re_h, im_h
        else:                    # relation: (re_h re_t + im_h im_t).Re_r + (re_h im_t - im_h re_t).Im_r
            assert re_r.dim() == 3 and re_h.dim() == 2 and re_t.dim() == 2
            A = E.ewise(E.EW_MULADD, re_h, re_t, im_h, im_t)
            Bq = E.ewise(E.EW_MULSUB, re_h, im_t, im_h, re_t)
            cre, cim = re_r, im_r
        tre, tim = _table_of(cre), _table_of(cim)
        if tre is not None and tim is not None:
            return E.LpProblem(E.LP_DOT, A, E.f32c(tre), A1=Bq, T1=E.f32c(tim)).scores()
        s = E.lp_scores_batched(E.LP_DOT, A, cre)
        return E.ewise(E.EW_ADD, s, E.lp_scores_batched(E.LP_DOT, Bq, cim))

    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """((re_h, im_h), (re_t, im_t), (re_r, im_r), (re_cand, im_cand))
        (bilinear.py:530-556)."""
        self._check_unsharded('inference_prepare_candidates')
        b_size = max(h_idx.shape[0], t_idx.shape[0], r_idx.shape[0])   # inference passes one empty index
        Ere, Eim, Rre, Rim = [x.data for x in self._tables()]
        g = _hip.gather_rows
        h = (g(Ere, h_idx), g(Eim, h_idx))
        t = (g(Ere, t_idx), g(Eim, t_idx))
        r = (g(Rre, r_idx), g(Rim, r_idx))
        if entities:
            shape = (b_size, self.n_ent, self.emb_dim)
            cand = (Ere.view(1, self.n_ent, self.emb_dim).expand(*shape),
                    Eim.view(1, self.n_ent, self.emb_dim).expand(*shape))
        else:
            shape = (b_size, self.n_rel, self.emb_dim)
            cand = (Rre.view(1, self.n_rel, self.emb_dim).expand(*shape),
                    Rim.view(1, self.n_rel, self.emb_dim).expand(*shape))
        return h, t, r, cand

    def one_vs_all_loss(self, h_idx, t_idx, r_idx, side='both', label_smoothing=0.0, reduction='mean'):
        """Softmax cross-entropy of every fact's true tail among ALL entities as tails of (h, r, ?) (``side='tail'``),
        of its true head among all heads of (?, r, t) (``'head'``), or both as one problem of 2B queries, the tail side
        first like ``lp_problem_both`` (``'both'``).  ``label_smoothing`` and ``reduction`` as torch's ``cross_entropy``.

        The scores are those of ``inference_scoring_function`` -- Re(<h, r, conj(c)>) as two segments over the
        [Re | Im] tables -- exactly what the evaluator ranks.  The (B, N) score matrix is never written
        (torchkge_amd.utils.one_vs_all).  The gradients of the entity tables are dense by nature -- every entity is a
        candidate of every query -- whatever ``row_gradients()`` says; so are the relation tables' here.  The query
        rows' part is summed by the ordered reduction under ``deterministic()``, the all-candidates part always in a
        fixed order."""
        return one_vs_all_loss(self, h_idx, t_idx, r_idx, side, label_smoothing, reduction)

    def k_vs_all_loss(self, ent_idx, r_idx, labels, side, label_smoothing=0.0, reduction='mean'):
        """Binary cross-entropy with logits of every key's scores over ALL entities against the set of its known
        answers: the keys are (h, r) = (``ent_idx``, ``r_idx``) scored against all tails (``side='tail'``) or (t, r)
        scored against all heads (``'head'``); ``labels = (seg_lo, seg_hi, targets)`` names each key's sorted answer
        list in place (``FilterIndex.lookup`` / ``.targets``).  ``reduction`` as torch's
        ``binary_cross_entropy_with_logits`` ('mean' divides by B * N); ``label_smoothing`` mixes every label with the
        uniform distribution over the entities (torchkge_amd.utils.k_vs_all).

        The scores are those of ``inference_scoring_function`` on the raw tables, exactly what the evaluator ranks, and
        neither the (B, N) score matrix nor a (B, N) label matrix is ever written.  The gradients of the tables are
        dense by nature; the query rows' part is summed by the ordered reduction under ``deterministic()``, the
        all-candidates part always in a fixed order."""
        return k_vs_all_loss(self, ent_idx, r_idx, labels, side, label_smoothing, reduction)

    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        tabs = [x.data for x in self._tables()]
        sd = _hip.side_code(side)
        if ent_lo == 0 and ent_hi == self.n_ent and self._row_shard is None and exchange is None and qtabs is None:
            prob = self._dot_fused_problem(sd, h_idx, t_idx, r_idx, [_hip.f32c(tabs[0]), _hip.f32c(tabs[1])],
                                           [_hip.f32c(tabs[2]), _hip.f32c(tabs[3])])
            if prob is not None:
                return prob
        Q0, Q1, _, _ = self._lp_prep(sd, h_idx, t_idx, r_idx, exchange, qtabs=qtabs, want_q1=True)
        T0, T1 = self._cand_rows(_hip.f32c(tabs[0]), ent_lo, ent_hi), self._cand_rows(_hip.f32c(tabs[1]), ent_lo, ent_hi)
        prob = self._attach_dot_split(_hip.LpProblem(_hip.LP_DOT, Q0, T0, A1=Q1, T1=T1, c_base=ent_lo), T0, T1,
                                      c_base=ent_lo)
        prob.cols = cols if (sd == _hip.SIDE_BOTH and prob.split is not None) else None
        return prob


class RelationOperators(object):
    """Light handle standing for the reference's (b, d, d) ``r_mat`` of RESCAL / HolE
    ``inference_prepare_candidates`` (bilinear.py:135, :398): the relation operator of each query, named by
    index instead of gathering b * d * d floats; ``materialize()`` gives the tensor itself."""

    def __init__(self, model, r_idx):
        self.model, self.r_idx = model, r_idx
        d = model.emb_dim
        self.shape = (r_idx.shape[0], d, d)

    def dim(self):
        return 3

    def materialize(self):
        return self.model._operators(self.r_idx)


class RelationOperatorTable(object):
    """Light handle standing for the reference's (b, n_rel, d, d) relation candidates of RESCAL / HolE
    (bilinear.py:137-140, :403-407: the operator of every relation, expanded over the batch);
    ``materialize()`` gives that stride-0 view."""

    def __init__(self, model, b_size):
        self.model = model
        d = model.emb_dim
        self.shape = (b_size, model.n_rel, d, d)

    def dim(self):
        return 4

    def materialize(self):
        m = self.model
        ops = m._operators(torch.arange(m.n_rel, device=m._tables()[1].device))
        return ops.view(1, *self.shape[1:]).expand(*self.shape)


def _ndim(x):
    return x.dim()


class _OperatorModel(BilinearModel):
    """Bilinear models whose relation is a d x d operator B_r: score = h . B_r . t (RESCAL: B_r = M_r, HolE: the
    rolling matrix of r).  The query rows h . B_r / B_r . t come from the relation-grouped transform
    (kge_bilinear_query); from there on every path is DistMult's KGE_LP_DOT against the entity table."""

    _ENT_TABLES = ('ent_emb',)

    def _tables(self):
        return [self.ent_emb.weight, self._rel_param().weight]

    def _lp_width(self):
        return self.emb_dim

    def normalize_parameters(self):
        """L2-normalise entity embeddings (bilinear.py:73-80, :342-349)."""
        self._normalize_weight_(self.ent_emb)

    def _queries(self, x, r, side):
        """(b, d) query rows x . B_r (side tail) or x . B_r^T (side head) for the rows ``x``; ``r`` is a
        RelationOperators handle or a real (b, d, d) tensor of operators."""
        b = x.shape[0]
        idx = torch.arange(b, device=x.device)
        sd = _hip.side_code(side)
        if isinstance(r, RelationOperators):
            return _hip.bilinear_query(self._kind, sd, x, _hip.f32c(self._rel_param().weight.data), idx, idx, r.r_idx)
        d = self.emb_dim
        one = r.shape[0] == 1 or r.stride(0) == 0        # one operator broadcast over the batch
        ops = r[:1].reshape(1, d * d) if one else r.reshape(b, d * d)
        return _hip.bilinear_query(_hip.RESCAL, sd, x, _hip.f32c(ops), idx, idx, torch.zeros_like(idx) if one else idx)

    def _relation_scores(self, h, t, cand):
        """(b, n_rel) scores of every relation: RESCAL vec(h t^T) . vec(M_rho), HolE c . R[rho] (c_k = sum_j h_j
        t_(j+k) mod d), both as KGE_LP_DOT against the relation table; a real (b, n_rel, d, d) candidate tensor is
        scored as matrices (vec(h t^T) . vec(cand[i, rho]))."""
        if isinstance(cand, RelationOperatorTable):
            rows = _hip.bilinear_relation_rows(self._kind, h, t)
            return _hip.LpProblem(_hip.LP_DOT, rows, _hip.f32c(self._rel_param().weight.data)).scores()
        b, n_rel, d = cand.shape[0], cand.shape[1], self.emb_dim
        rows = _hip.bilinear_relation_rows(_hip.RESCAL, h, t)
        if cand.stride(0) == 0 or b == 1:
            return _hip.LpProblem(_hip.LP_DOT, rows, _hip.f32c(cand[0].reshape(n_rel, d * d))).scores()
        return _hip.lp_scores_batched(_hip.LP_DOT, rows, _hip.f32c(cand.reshape(b, n_rel, d * d)))

    def inference_scoring_function(self, h, t, r):
        """Rank dispatch of bilinear.py:98-121 / :365-389: the 3-D entity argument is the candidate set (with the
        (b, d, d) operators in ``r``); a 4-D ``r`` means relation candidates."""
        if _ndim(r) == 4:
            assert _ndim(h) == 2 and _ndim(t) == 2
            return self._relation_scores(h, t, r)
        assert _ndim(r) == 3
        if _ndim(t) == 3:
            assert _ndim(h) == 2                     # tail completion: (h . B_r) . cand
            q, cand = self._queries(h, r, 'tail'), t
        else:
            assert _ndim(h) == 3 and _ndim(t) == 2  # head completion: (B_r . t) . cand
            q, cand = self._queries(t, r, 'head'), h
        table = _table_of(cand)
        if table is not None:
            return _hip.LpProblem(_hip.LP_DOT, q, _hip.f32c(table)).scores()
        return _hip.lp_scores_batched(_hip.LP_DOT, q, _hip.f32c(cand))

    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """(h, t, r_mat, candidates) (bilinear.py:123-143, :391-411): r_mat is a RelationOperators handle for the
        (b, d, d) operators, candidates a stride-0 (b, n_ent, d) view of the entity table or a RelationOperatorTable
        handle for the (b, n_rel, d, d) relation operators."""
        self._check_unsharded('inference_prepare_candidates')
        b_size = max(h_idx.shape[0], t_idx.shape[0], r_idx.shape[0])   # inference passes one empty index
        E = self.ent_emb.weight.data
        h, t = _hip.gather_rows(E, h_idx), _hip.gather_rows(E, t_idx)
        r = RelationOperators(self, r_idx)
        if entities:
            candidates = E.view(1, self.n_ent, self.emb_dim).expand(b_size, self.n_ent, self.emb_dim)
        else:
            candidates = RelationOperatorTable(self, b_size)
        return h, t, r, candidates

    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        sd = _hip.side_code(side)
        Q0 = self._lp_prep(sd, h_idx, t_idx, r_idx, exchange, qtabs=qtabs)[0]
        T0 = self._cand_rows(_hip.f32c(self.ent_emb.weight.data), ent_lo, ent_hi)
        prob = self._attach_dot_split(_hip.LpProblem(_hip.LP_DOT, Q0, T0, c_base=ent_lo), T0, c_base=ent_lo)
        prob.cols = cols if (sd == _hip.SIDE_BOTH and prob.split is not None) else None
        return prob


class RESCALModel(_OperatorModel):
    """RESCAL (bilinear.py:14-143): ``RESCALModel(emb_dim, n_entities, n_relations)``; parameters ``ent_emb``
    (L2-normalised rows) and ``rel_mat`` (n_rel, emb_dim * emb_dim), M_r = rel_mat[r].view(d, d)."""

    _kind = _hip.RESCAL
    _DENSE_GRAD_TABLES = ('rel_mat',)       # reduced per relation by kge_rescal_rel_grad: not row-shaped

    def __init__(self, emb_dim, n_entities, n_relations):
        super().__init__(emb_dim, n_entities, n_relations)
        self.ent_emb = init_embedding(self.n_ent, self.emb_dim)
        self.rel_mat = init_embedding(self.n_rel, self.emb_dim * self.emb_dim)
        self.ent_emb.weight.data = torch.nn.functional.normalize(self.ent_emb.weight.data, p=2, dim=1)

    def _rel_param(self):
        return self.rel_mat

    def _operators(self, r_idx):
        d = self.emb_dim
        return _hip.gather_rows(self.rel_mat.weight.data, r_idx).view(-1, d, d)

    def get_embeddings(self):
        """(ent_emb, rel_mat viewed (n_rel, d, d)) (bilinear.py:82-96)."""
        self.normalize_parameters()
        return self.ent_emb.weight.data, self.rel_mat.weight.data.view(-1, self.emb_dim, self.emb_dim)


class HolEModel(_OperatorModel):
    """HolE (bilinear.py:270-411): ``HolEModel(emb_dim, n_entities, n_relations)``; parameters ``ent_emb``
    (L2-normalised rows) and ``rel_emb``; B_r = get_rolling_matrix(rel_emb[r])."""

    _kind = _hip.HOLE

    def __init__(self, emb_dim, n_entities, n_relations):
        super().__init__(emb_dim, n_entities, n_relations)
        self.ent_emb = init_embedding(self.n_ent, self.emb_dim)
        self.rel_emb = init_embedding(self.n_rel, self.emb_dim)
        self.ent_emb.weight.data = torch.nn.functional.normalize(self.ent_emb.weight.data, p=2, dim=1)

    def _rel_param(self):
        return self.rel_emb

    @staticmethod
    def get_rolling_matrix(x):
        """(b, d) -> (b, d, d) with mat[i, j, k] = x[i, (k - j) mod d] (bilinear.py:326-340); any device."""
        b_size, dim = x.shape
        ar = torch.arange(dim, device=x.device)
        idx = (ar.view(1, dim) - ar.view(dim, 1)) % dim
        return x[:, idx.view(-1)].view(b_size, dim, dim)

    def _operators(self, r_idx):
        return self.get_rolling_matrix(_hip.gather_rows(self.rel_emb.weight.data, r_idx))

    def get_embeddings(self):
        """(ent_emb, rel_emb) (bilinear.py:351-363)."""
        self.normalize_parameters()
        return self.ent_emb.weight.data, self.rel_emb.weight.data


class _AnalogyScore(torch.autograd.Function):
    """ANALOGY's scoring_function as one fused HIP kernel, differentiable wrt the six tables
    (kge_analogy_score_triples / _bwd + the sorted row reduction)."""

    @staticmethod
    def forward(ctx, h, t, r, *tables):
        tabs = [x.detach() for x in tables]
        ctx.row_grads = is_row_gradients()      # read here: a loss built inside row_gradients() keeps the mode
        ctx.save_for_backward(h, t, r, *tabs)
        return _hip_analogy.score_triples(tabs[:3], tabs[3:], h, t, r)

    @staticmethod
    def backward(ctx, grad_out):
        h, t, r = ctx.saved_tensors[:3]
        tabs = list(ctx.saved_tensors[3:])
        grads = _hip_analogy.score_triples_bwd(tabs[:3], tabs[3:], h, t, r, grad_out, ctx.needs_input_grad[3:], row_grads=ctx.row_grads)
        return (None,) * 3 + tuple(grads)


class AnalogyModel(BilinearModel):
    """ANALOGY (bilinear.py:559-763): ``AnalogyModel(emb_dim, n_entities, n_relations, scalar_share=0.5)``; DistMult on
    ``scalar_dim = int(emb_dim * scalar_share)`` coordinates plus ComplEx on ``complex_dim = emb_dim - scalar_dim``;
    parameters ``sc_ent_emb``, ``re_ent_emb``, ``im_ent_emb``, ``sc_rel_emb``, ``re_rel_emb``, ``im_rel_emb``; never
    normalised (:652-656).

    The score against a candidate is ONE dot product of width K = scalar_dim + 2 complex_dim between a query row
    (kge_analogy_query) and the candidate's packed row [sc | re | im] (kge_analogy_pack_rows, once per evaluation): from
    there on every path is DistMult's one-segment KGE_LP_DOT.  The documented score is served for EVERY split; the
    reference's own inference_scoring_function adds (b, N, scalar_dim) to (b, N, complex_dim) tensors and so raises
    (or broadcasts) unless the two are equal."""

    _kind = None            # no kind of include/kge_hip.h: the entry points are those of include/kge_hip_analogy.h
    _ENT_TABLES = ('sc_ent_emb', 're_ent_emb', 'im_ent_emb')
    _ENT_POS = (0, 1, 2)

    def __init__(self, emb_dim, n_entities, n_relations, scalar_share=0.5):
        super().__init__(emb_dim, n_entities, n_relations)
        self.scalar_dim = int(self.emb_dim * scalar_share)
        self.complex_dim = int(self.emb_dim - self.scalar_dim)
        if self.scalar_dim > _hip_analogy.MAX_DIM or self.complex_dim > _hip_analogy.MAX_DIM:
            raise RuntimeError('torchkge_amd: AnalogyModel handles scalar_dim, complex_dim <= %d' % _hip_analogy.MAX_DIM)
        self.sc_ent_emb = init_embedding(self.n_ent, self.scalar_dim)
        self.re_ent_emb = init_embedding(self.n_ent, self.complex_dim)
        self.im_ent_emb = init_embedding(self.n_ent, self.complex_dim)
        self.sc_rel_emb = init_embedding(self.n_rel, self.scalar_dim)
        self.re_rel_emb = init_embedding(self.n_rel, self.complex_dim)
        self.im_rel_emb = init_embedding(self.n_rel, self.complex_dim)

    def _tables(self):
        return [self.sc_ent_emb.weight, self.re_ent_emb.weight, self.im_ent_emb.weight,
                self.sc_rel_emb.weight, self.re_rel_emb.weight, self.im_rel_emb.weight]

    def _penalty_groups(self):
        """The scalar tables element by element, the complex part by the modulus of a coordinate, on both sides."""
        from .._hip_penalty import REAL, SPLIT
        return ([(REAL, self.sc_ent_emb.weight), (SPLIT, (self.re_ent_emb.weight, self.im_ent_emb.weight))],
                [(REAL, self.sc_rel_emb.weight), (SPLIT, (self.re_rel_emb.weight, self.im_rel_emb.weight))])

    def _lp_width(self):
        return self.scalar_dim + 2 * self.complex_dim

    def normalize_parameters(self):
        """No normalisation for ANALOGY (bilinear.py:652-656)."""
        pass

    def get_embeddings(self):
        return tuple(x.data for x in self._tables())

    def scoring_function(self, h_idx, t_idx, r_idx):
        """sc_h . diag(sc_r) . sc_t + Re(<h, r, conj(t)>) of each triplet (bilinear.py:634-650), one fused HIP kernel,
        differentiable."""
        self._check_unsharded('scoring_function')
        tables = self._tables()
        _hip.require_cuda(h_idx, t_idx, r_idx, *tables)
        return _AnalogyScore.apply(h_idx, t_idx, r_idx, *tables)

    # ---- the packed candidate rows ----------------------------------------
    def _packed(self, name, tabs):
        """(rows, K rounded up to 4) packed [sc | re | im] rows of the three tables ``tabs``, pads zero: built once per
        lp_session (never kept across sessions: the tables may change between them); inside a captured evaluation the
        pack launch is part of the graph and reads the parameters at their addresses."""
        tabs = [_hip.f32c(x) for x in tabs]
        return self._cache.get(name, tabs, lambda: _hip_analogy.pack_rows(tabs))

    def _dot(self, q, P):
        return _hip.LpProblem(_hip.LP_DOT, q, P, K0=self._lp_width())

    def inference_scoring_function(self, h, t, r):
        """h, t, r are (sc, re, im) tuples; the one holding 3-D tensors is the candidate set (bilinear.py:682-711)."""
        A = _hip_analogy
        if t[1].dim() == 3:
            assert h[1].dim() == 2 and r[1].dim() == 2      # tail completion
            q, cand = A.query(_hip.SIDE_TAIL, h, r, None, None, None, B=h[1].shape[0]), t
        elif h[1].dim() == 3:
            assert t[1].dim() == 2 and r[1].dim() == 2      # head completion
            q, cand = A.query(_hip.SIDE_HEAD, t, r, None, None, None, B=t[1].shape[0]), h
        else:
            assert r[1].dim() == 3 and h[1].dim() == 2 and t[1].dim() == 2      # relation prediction
            q, cand = A.query(A.SIDE_REL, h, t, None, None, None, B=h[1].shape[0]), r
        tabs = [_table_of(c) for c in cand]
        if all(x is not None for x in tabs):
            return self._dot(q, self._packed('apk_cand', tabs)).scores()
        # real materialised candidates: one batched product per segment, summed
        d_sc, d_c = self.scalar_dim, self.complex_dim
        s = None
        for c0, w, c in ((0, d_sc, cand[0]), (d_sc, d_c, cand[1]), (d_sc + d_c, d_c, cand[2])):
            if w:
                part = _hip.lp_scores_batched(_hip.LP_DOT, q[:, c0:c0 + w], c)
                s = part if s is None else _hip.ewise(_hip.EW_ADD, s, part)
        return s

    def inference_prepare_candidates(self, h_idx, t_idx, r_idx, entities=True):
        """((sc_h, re_h, im_h), (sc_t, re_t, im_t), (sc_r, re_r, im_r), (sc_cand, re_cand, im_cand)) with stride-0
        candidate views (bilinear.py:713-763)."""
        self._check_unsharded('inference_prepare_candidates')
        b_size = max(h_idx.shape[0], t_idx.shape[0], r_idx.shape[0])   # inference passes one empty index
        tabs = [x.data for x in self._tables()]
        ent, rel = tabs[:3], tabs[3:]
        K = self._lp_width()
        d_sc, d_c = self.scalar_dim, self.complex_dim

        def rows(tt, idx):      # the three gathers as one pack launch, handed out as column slices
            P = _hip_analogy.pack_rows(tt, idx)
            return P[:, :d_sc], P[:, d_sc:d_sc + d_c], P[:, d_sc + d_c:K]
        h, t, r = rows(ent, h_idx), rows(ent, t_idx), rows(rel, r_idx)
        src, n = (ent, self.n_ent) if entities else (rel, self.n_rel)
        cand = tuple(x.view(1, n, x.shape[1]).expand(b_size, n, x.shape[1]) for x in src)
        return h, t, r, cand

    # ---- evaluation ---------------------------------------------------------
    def _lp_prep(self, side, h_idx, t_idx, r_idx, exchange=None, qtabs=None, **want):
        """The query rows of a batch (kge_analogy_query).  Row-sharded tables: rows of entities another rank owns come
        back as zeros and ``exchange`` sums them over the shards; ``qtabs``: the three query-entity replicas replace the
        entity tables (h_idx / t_idx index them)."""
        tabs = [x.data for x in self._tables()]
        ent, rel = tabs[:3], tabs[3:]
        if qtabs is not None:
            return (_hip_analogy.query(side, list(qtabs), rel, h_idx, t_idx, r_idx),)
        lo, n = (self._row_shard[0], self._row_shard[1] - self._row_shard[0]) if self._row_shard is not None else (0, -1)
        Q = _hip_analogy.query(side, ent, rel, h_idx, t_idx, r_idx, ent_lo=lo, ent_n=n)
        if self._row_shard is not None:
            if exchange is None:
                raise RuntimeError('torchkge_amd: a row-sharded model needs the evaluator\'s query exchange')
            exchange([Q])
        return (Q,)

    def lp_problem(self, h_idx, t_idx, r_idx, side, ent_lo=0, ent_hi=None, exchange=None, qtabs=None, cols=None):
        ent_lo, ent_hi = _ent_range(self, ent_lo, ent_hi)
        sd = _hip.side_code(side)
        K = self._lp_width()
        Q = self._lp_prep(sd, h_idx, t_idx, r_idx, exchange, qtabs=qtabs)[0]
        ent = [self._cand_rows(x.data, ent_lo, ent_hi) for x in self._tables()[:3]]
        P = self._packed('apk_%d_%d' % (ent_lo, ent_hi), ent)
        prob = self._attach_dot_split(_hip.LpProblem(_hip.LP_DOT, Q, P, c_base=ent_lo, K0=K), P, c_base=ent_lo, K=K)
        prob.cols = cols if (sd == _hip.SIDE_BOTH and prob.split is not None) else None
        return prob

    def lp_true_scores_replica(self, prob, qctx):
        """The (2B) true scores from the query-entity replicas, on every rank: the replicas packed (once per evaluation)
        and the one-segment DOT problem's pair chain -- the rows and the chain the owner shard runs: identical bits."""
        qt, hq, tq = qctx
        P = self._packed('apk_replica', list(qt))
        return self._dot(prob.keep[0], P).pair_scores(torch.cat([tq, hq]))
