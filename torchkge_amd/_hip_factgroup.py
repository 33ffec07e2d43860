# -*- coding: utf-8 -*-
"""ctypes binding of the grouped scorer of libkge_hip.so (include/kge_hip_factgroup.h): ``score_fact_groups`` -- the
scores of B facts and of the K negatives of each from one kge_score_fact_groups, a fact's rows gathered once --
``score_fact_groups_bwd`` -- its gradient rows, reduced into dense tables or handed on as uncoalesced sparse gradients --
and the ``torch.autograd.Function`` around the two (``ScoreFactGroups``).

The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature table of
their own because include/kge_hip.h and its ABI version do not change for them.  Nothing here synchronises or reads
back."""
import ctypes

import torch

from . import _hip, _hip_det
from ._hip import _vp, _i64, _int, _check, _on, _p, _stream, f32c, i64c

_size = ctypes.c_size_t
_SIGNATURES = {
    'kge_score_fact_groups': [_int, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp],
    'kge_score_fact_groups_bwd': [_int, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64,
                                  _vp, _i64, _vp, _vp],
    'kge_fact_group_entity_tables': [_int],
    'kge_fact_group_relation_tables': [_int],
    'kge_fact_group_forward_chunks': [_i64],
}
WAVES, K_PER_CHUNK, MAX_CHUNKS = 4, 128, 1024       # KGE_FACT_GROUP_* of the header
# the kind's tables (positions in Model._tables()) in the order of the rows buffer's blocks: (entity tables, relation tables)
_DEFAULT_TABLES = ((0,), (1,))
_TABLES = {_hip.TRANSH: ((0,), (1, 2)), _hip.COMPLEX: ((0, 1), (2, 3)), _hip.TRANSD: ((0, 2), (1, 3))}
KINDS = frozenset([_hip.TRANSE_L1, _hip.TRANSE_L2, _hip.TRANSH, _hip.TRANSD, _hip.DISTMULT, _hip.COMPLEX, _hip.TORUSE_L1,
                   _hip.TORUSE_TORUS_L1, _hip.TORUSE_TORUS_L2, _hip.TORUSE_TORUS_EL2])


class Unsupported(Exception):
    """kge_score_fact_groups answered KGE_EUNSUPPORTED: nothing was launched, the caller takes the general path."""


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    lib = _hip.bind(_SIGNATURES)
    lib.kge_fact_group_rows_per_fact.argtypes, lib.kge_fact_group_rows_per_fact.restype = [_int, _i64], _i64
    lib.kge_fact_group_rows.argtypes, lib.kge_fact_group_rows.restype = [_int, _i64, _i64], _i64
    lib.kge_fact_group_rows_bytes.argtypes, lib.kge_fact_group_rows_bytes.restype = [_int, _i64, _i64, _i64], _size
    lib.kge_fact_group_ids.argtypes, lib.kge_fact_group_ids.restype = [_i64, _i64], _i64
    return lib


def tables_of(kind):
    """(entity tables, relation tables) of ``kind``: positions in the model's table list, in the order of the blocks of
    the rows buffer."""
    return _TABLES.get(kind, _DEFAULT_TABLES)


def rows_per_fact(kind, K):
    """kge_fact_group_rows_per_fact: host arithmetic."""
    return int(load_library().kge_fact_group_rows_per_fact(kind, K))


def _groups(h, neg_h, neg_t):
    B = h.shape[0]
    if neg_h.shape[0] != neg_t.shape[0] or (B == 0 and neg_h.shape[0] != 0) or (B > 0 and neg_h.shape[0] % B != 0):
        raise ValueError('torchkge_amd: %d / %d negative heads / tails are not a whole number per fact of %d facts'
                         % (neg_h.shape[0], neg_t.shape[0], B))
    return B, (neg_h.shape[0] // B if B else 1)


def score_fact_groups(kind, tables, d_ent, d_rel, h, t, r, neg_h, neg_t):
    """kge_score_fact_groups on the current stream: ``(pos, neg)`` -- the B scores of the facts and the K * B scores of
    their negatives in tile order (negative k of fact i at k * B + i), each with the bits kge_score_triples gives the
    same triple.  Raises ``Unsupported`` where the library answers KGE_EUNSUPPORTED (rows wider than 512 floats)."""
    lib = load_library()
    _hip.require_cuda(h, t, r, neg_h, neg_t, *tables)
    tabs = [f32c(x) for x in tables] + [None] * (4 - len(tables))
    h, t, r, neg_h, neg_t = (i64c(x) for x in (h, t, r, neg_h, neg_t))
    B, K = _groups(h, neg_h, neg_t)
    pos = torch.empty(B, dtype=torch.float32, device=h.device)
    neg = torch.empty(K * B, dtype=torch.float32, device=h.device)
    with _on(h.device):
        rc = lib.kge_score_fact_groups(kind, _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(tabs[3]), d_ent, d_rel, _p(h), _p(t),
                                       _p(r), B, _p(neg_h), _p(neg_t), K, _p(pos), _p(neg), max(B, 1), _stream())
    if rc == _hip.KGE_EUNSUPPORTED:
        raise Unsupported()
    _check(rc, 'kge_score_fact_groups')
    return pos, neg


def fact_group_rows(kind, tables, d_ent, d_rel, h, t, r, neg_h, neg_t, go_pos, go_neg):
    """kge_score_fact_groups_bwd on the current stream: ``(rows, ids, ld)`` -- the rows buffer of the header's layout as
    one float32 vector (rows ``ld`` floats apart), and the B (K + 2) target ids of an entity table's block."""
    lib = load_library()
    tabs = [f32c(x) for x in tables] + [None] * (4 - len(tables))
    B, K = _groups(h, neg_h, neg_t)
    dev, ld = h.device, d_ent
    rows = torch.empty(int(lib.kge_fact_group_rows(kind, B, K)) * ld, dtype=torch.float32, device=dev)
    ids = torch.empty(B * (K + 2), dtype=torch.int64, device=dev)
    with _on(dev):
        _check(lib.kge_score_fact_groups_bwd(kind, _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(tabs[3]), d_ent, d_rel, _p(h),
                                             _p(t), _p(r), B, _p(neg_h), _p(neg_t), K, _p(go_pos), _p(go_neg), max(B, 1),
                                             _p(rows), ld, _p(ids), _stream()), 'kge_score_fact_groups_bwd')
    return rows, ids, ld


def score_fact_groups_bwd(kind, tables, d_ent, d_rel, h, t, r, neg_h, neg_t, go_pos, go_neg, needs, row_grads=False):
    """The gradients of ``tables`` (None where ``needs`` is False).  Dense tables through _hip_det.reduce_rows -- one
    sort of the B (K + 2) entity ids and one of the B relation ids, in default and in deterministic mode -- or, with
    ``row_grads`` (torchkge_amd.rowgrad, as the forward read it), uncoalesced sparse gradients whose values are views of
    the rows buffer: B (K + 2) rows per entity table, B per relation table, not reduced."""
    from ._hip_rows import sparse_rows
    h, t, r, neg_h, neg_t = (i64c(x) for x in (h, t, r, neg_h, neg_t))
    B, K = _groups(h, neg_h, neg_t)
    tabs = [f32c(x) for x in tables]
    grads = [None] * len(tabs)
    if B == 0:
        return [torch.zeros_like(x) if n else None for x, n in zip(tabs, needs)]
    rows, ids, ld = fact_group_rows(kind, tabs, d_ent, d_rel, h, t, r, neg_h, neg_t, f32c(go_pos), f32c(go_neg))
    ent, rel = tables_of(kind)
    n_ent_rows = (K + 2) * B
    blocks = [(ti, s * n_ent_rows, n_ent_rows, ids) for s, ti in enumerate(ent)]
    blocks += [(ti, len(ent) * n_ent_rows + q * B, B, r) for q, ti in enumerate(rel)]
    det = _hip_det.is_deterministic()
    perms = {}
    with _on(h.device):
        for ti, row0, n, keys in blocks:
            if not needs[ti]:
                continue
            d = tabs[ti].shape[1]
            if row_grads:
                vals = rows[row0 * ld:(row0 + n) * ld].view(n, ld)
                grads[ti] = sparse_rows(keys, vals if ld == d else vals[:, :d].contiguous(), tabs[ti].shape)
            else:
                g = grads[ti] = torch.zeros_like(tabs[ti])
                perms[id(keys)] = _hip_det.reduce_rows(rows.data_ptr() + row0 * ld * 4, ld, d, keys, None, g,
                                                       perm=perms.get(id(keys)), det=det)
    return grads


class ScoreFactGroups(torch.autograd.Function):
    """pos, neg = ScoreFactGroups.apply(kind, d_ent, d_rel, h, t, r, neg_h, neg_t, *tables): differentiable with respect
    to the tables."""

    @staticmethod
    def forward(ctx, kind, d_ent, d_rel, h, t, r, neg_h, neg_t, *tables):
        from .rowgrad import is_row_gradients
        tabs = [x.detach() for x in tables]
        ctx.kind, ctx.d_ent, ctx.d_rel = kind, d_ent, d_rel
        ctx.row_grads = is_row_gradients()      # read here: a loss built inside row_gradients() keeps the mode
        pos, neg = score_fact_groups(kind, tabs, d_ent, d_rel, h, t, r, neg_h, neg_t)
        ctx.save_for_backward(h, t, r, neg_h, neg_t, *tabs)
        return pos, neg

    @staticmethod
    def backward(ctx, go_pos, go_neg):
        h, t, r, neg_h, neg_t = ctx.saved_tensors[:5]
        tabs = list(ctx.saved_tensors[5:])
        grads = score_fact_groups_bwd(ctx.kind, tabs, ctx.d_ent, ctx.d_rel, h, t, r, neg_h, neg_t, go_pos, go_neg,
                                      ctx.needs_input_grad[8:], row_grads=ctx.row_grads)
        return (None,) * 8 + tuple(grads)
