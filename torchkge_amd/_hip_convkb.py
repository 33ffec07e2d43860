# -*- coding: utf-8 -*-
"""ctypes binding of the ConvKB entry points of libkge_hip.so (include/kge_hip_convkb.h) and their tensor-level
wrappers.  The symbols live in the library _hip.load_library() returns; their prototypes have a header and a signature
table of their own because include/kge_hip.h, kge_lp_desc and its ABI version do not change for this model.

``ConvKBProblem`` has the surface the evaluator and EntityInference use on ``_hip.LpProblem``.  Nothing in a launch path
synchronises or reads back: evaluate() captures these launches into its hipGraph."""
import ctypes

import torch

from . import _hip, _hip_det
from ._hip_rows import sparse_rows
from ._hip import _vp, _i64, _int, _p, _check, _on, _stream, f32c, f32rows, i64c, require_cuda

MAX_DIM = 512       # KGE_CONVKB_MAX_DIM: of each of d (emb_dim) and F (n_filters)
SLOT_HEAD, SLOT_REL, SLOT_TAIL, SLOT_BOTH = 0, 1, 2, 3      # the slot the candidates fill; KGE_CONVKB_SLOT_BOTH
TILE_Q, TILE_C = 4, 1024    # queries / candidates per workgroup tile of the score / count kernel (csrc/convkb.hip)


class ConvKBDesc(ctypes.Structure):
    """kge_convkb_desc."""
    _fields_ = [('slot', ctypes.c_int32), ('d', ctypes.c_int32), ('F', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('B', _i64), ('N', _i64), ('c_base', _i64), ('B_tail', _i64),
                ('QE', _vp), ('ld_qe', _i64), ('qe_idx', _vp),
                ('QR', _vp), ('ld_qr', _i64), ('qr_idx', _vp),
                ('T', _vp), ('ldt', _i64),
                ('D', _vp), ('Dt', _vp), ('wp', _vp), ('db', _vp)]


_SIGNATURES = {
    'kge_convkb_prepare': [_vp, _vp, _vp, _i64, _vp, _int, _int, _vp, _vp],
    'kge_convkb_scores': [_vp, _vp, _i64, _vp],
    'kge_convkb_pair_scores': [_vp, _vp, _vp, _i64, _vp, _vp],
    'kge_convkb_count_ge': [_vp, _vp, _vp, _vp],
    'kge_convkb_filter_sub': [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'kge_convkb_score_triples': [_vp, _i64, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _i64, _vp, _vp],
    'kge_convkb_score_triples_bwd': [_vp, _i64, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64,
                                     _vp, _vp, _vp, _vp, _vp],
}


def load_library():
    """The handle of _hip.load_library() with the argtypes of this header bound."""
    return _hip.bind(_SIGNATURES)


def check_dims(d, F):
    if not (1 <= d <= MAX_DIM and 1 <= F <= MAX_DIM):
        raise RuntimeError('torchkge_amd: ConvKBModel handles 1 <= emb_dim <= %d and 1 <= n_filters <= %d, got emb_dim = %d, '
                           'n_filters = %d' % (MAX_DIM, MAX_DIM, d, F))


def ws_floats(d, F):
    return 2 * d * F + 4 * F + 4        # KGE_CONVKB_WS_FLOATS


def prepare(conv_w, conv_b, lin_w, lin_b, d):
    """kge_convkb_prepare: the workspace [wp | db | D | Dt] of the four layer parameters (conv weight (F, 3, 1), conv
    bias (F), linear weight (2, F d), linear bias (2)).  One launch, no synchronisation."""
    lib = load_library()
    F = conv_w.shape[0]
    check_dims(d, F)
    w, cb, L, lb = f32c(conv_w), f32c(conv_b), f32rows(lin_w), f32c(lin_b)
    require_cuda(w, cb, L, lb)
    if tuple(L.shape) != (2, F * d) or w.numel() != 3 * F or cb.numel() != F or lb.numel() != 2:
        raise RuntimeError('torchkge_amd: ConvKB layer shapes do not fit emb_dim = %d, n_filters = %d' % (d, F))
    ws = torch.empty(ws_floats(d, F), dtype=torch.float32, device=w.device)
    with _on(ws.device):
        _check(lib.kge_convkb_prepare(_p(w), _p(cb), _p(L), L.stride(0), _p(lb), d, F, _p(ws), _stream()),
               'kge_convkb_prepare')
    return ws


class ConvKBProblem(object):
    """Python owner of a kge_convkb_desc: keeps the tensors alive and exposes the descriptor entry points with the
    surface of _hip.LpProblem.  ``QE`` / ``QR``: the two query-row matrices with their optional index vectors (see the
    header); ``T``: the candidate rows, local candidate c = global id c_base + c; ``ws``: prepare()'s workspace."""

    def __init__(self, slot, QE, qe_idx, QR, qr_idx, T, ws, d, F, B, c_base=0, B_tail=0):
        QE, QR, T = f32rows(QE), f32rows(QR), f32rows(T)
        qe_idx = None if qe_idx is None else i64c(qe_idx)
        qr_idx = None if qr_idx is None else i64c(qr_idx)
        require_cuda(QE, QR, T, ws, qe_idx, qr_idx)
        check_dims(d, F)
        self.keep = [QE, qe_idx, QR, qr_idx, T, ws]
        self.device = T.device
        p = ConvKBDesc()
        p.slot, p.d, p.F, p.reserved = slot, d, F, 0
        p.B, p.N, p.c_base, p.B_tail = B, T.shape[0], c_base, B_tail
        p.QE, p.ld_qe, p.qe_idx = QE.data_ptr(), QE.stride(0), (0 if qe_idx is None else qe_idx.data_ptr())
        p.QR, p.ld_qr, p.qr_idx = QR.data_ptr(), QR.stride(0), (0 if qr_idx is None else qr_idx.data_ptr())
        p.T, p.ldt = T.data_ptr(), T.stride(0)
        base = ws.data_ptr()
        p.wp, p.db = base, base + 4 * (4 * F)
        p.D = base + 4 * (4 * F + 4)
        p.Dt = p.D + 4 * d * F
        self.desc = p
        self.B, self.N = int(B), int(T.shape[0])
        self.split = self.sad = self.pre = self.cols = None     # (no prefilter, no fused query pipeline, no columns)

    def _copy(self):
        return ConvKBDesc.from_buffer_copy(self.desc)

    def scores(self, out=None):
        lib = load_library()
        if out is None:
            out = torch.empty(self.B, self.N, dtype=torch.float32, device=self.device)
        with _on(self.device):
            _check(lib.kge_convkb_scores(ctypes.byref(self.desc), _p(out), out.stride(0), _stream()), 'kge_convkb_scores')
        return out

    def scores_chunk(self, c0, c1, out):
        """Scores of LOCAL candidates [c0, c1) only, into out[:, :c1 - c0]: the descriptor with its candidate side advanced."""
        lib = load_library()
        p = self._copy()
        p.N, p.c_base = c1 - c0, self.desc.c_base + c0
        p.T = self.desc.T + 4 * c0 * self.desc.ldt
        with _on(self.device):
            _check(lib.kge_convkb_scores(ctypes.byref(p), _p(out), out.stride(0), _stream()), 'kge_convkb_scores')
        return out

    def scores_rows(self, q0, q1, out):
        """Scores of QUERIES [q0, q1) against every local candidate, into out[:q1 - q0]: the query side advanced."""
        lib = load_library()
        p = self._copy()
        p.B = q1 - q0
        p.B_tail = max(0, min(int(self.desc.B_tail) - q0, q1 - q0))
        if self.desc.qe_idx:
            p.qe_idx = self.desc.qe_idx + 8 * q0
        else:
            p.QE = self.desc.QE + 4 * q0 * self.desc.ld_qe
        if self.desc.qr_idx:
            p.qr_idx = self.desc.qr_idx + 8 * q0
        else:
            p.QR = self.desc.QR + 4 * q0 * self.desc.ld_qr
        if q1 > q0 and self.N > 0:
            with _on(self.device):
                _check(lib.kge_convkb_scores(ctypes.byref(p), _p(out), out.stride(0), _stream()), 'kge_convkb_scores')
        return out

    def pair_scores(self, ci, qi=None):
        lib = load_library()
        ci = i64c(ci)
        qi = None if qi is None else i64c(qi)
        P = ci.shape[0]
        out = torch.empty(P, dtype=torch.float32, device=self.device)
        with _on(self.device):
            _check(lib.kge_convkb_pair_scores(ctypes.byref(self.desc), _p(qi), _p(ci), P, _p(out), _stream()),
                   'kge_convkb_pair_scores')
        return out

    def count_ge(self, s_true, raw=None):
        lib = load_library()
        if raw is None:
            raw = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        with _on(self.device):
            _check(lib.kge_convkb_count_ge(ctypes.byref(self.desc), _p(s_true), _p(raw), _stream()), 'kge_convkb_count_ge')
        return raw

    def filter_sub(self, s_true, true_idx, seg_lo, seg_hi, targets, sub=None, found=None, grouped=False, plan=None):
        """Filter correction of every query (``grouped`` / ``plan``, the load-balanced forms of LpProblem, are ignored:
        one kernel, 8 lanes per query)."""
        lib = load_library()
        if sub is None:
            sub = torch.empty(self.B, dtype=torch.int32, device=self.device)
        if found is None:
            found = torch.empty(self.B, dtype=torch.int32, device=self.device)
        with _on(self.device):
            _check(lib.kge_convkb_filter_sub(ctypes.byref(self.desc), _p(s_true), _p(true_idx), _p(seg_lo), _p(seg_hi),
                                             _p(targets), _p(sub), _p(found), _stream()), 'kge_convkb_filter_sub')
        return sub, found


def score_triples(E, R, ws, d, F, h, t, r):
    lib = load_library()
    E, R = f32rows(E), f32rows(R)
    h, t, r = i64c(h), i64c(t), i64c(r)
    require_cuda(E, R, ws, h, t, r)
    B = h.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=h.device)
    with _on(h.device):
        _check(lib.kge_convkb_score_triples(_p(E), E.stride(0), _p(R), R.stride(0), d, F, _p(ws), _p(h), _p(t), _p(r), B,
                                            _p(out), _stream()), 'kge_convkb_score_triples')
    return out


def score_triples_bwd(E, R, ws, d, F, h, t, r, s, grad_out, needs, row_grads=False):
    """Gradients of (ent_emb, rel_emb, conv weight (F, 3, 1), conv bias, linear weight (2, F d), linear bias), None
    where ``needs`` says so.  Entity / relation gradients: per-triple rows reduced by _hip_det.reduce_rows
    (kge_key_sort, then kge_segment_sum_rows, or kge_segment_sum_ordered in deterministic mode; no per-element
    atomics); the four layer gradients: one reduction kernel over the batch (fixed-shape trees: the same bits on every run).
    ``row_grads`` (torchkge_amd.rowgrad, as the forward read it): no reduction -- the entity / relation gradients are the
    uncoalesced sparse tensors of the ids and views of the rows; the layer gradients stay dense."""
    lib = load_library()
    E, R = f32rows(E), f32rows(R)
    h, t, r = i64c(h), i64c(t), i64c(r)
    s, go = f32c(s), f32c(grad_out)
    B, dev = h.shape[0], h.device
    want_rows, want_par = any(needs[:2]), any(needs[2:])
    g = torch.empty(max(B, 1), dtype=torch.float32, device=dev)
    rows = torch.empty(3 * B, d, dtype=torch.float32, device=dev) if want_rows else None
    dL = dlb = dw = dcb = None
    if want_par:
        dL = torch.empty(2, F * d, dtype=torch.float32, device=dev)
        dlb = torch.empty(2, dtype=torch.float32, device=dev)
        dw = torch.empty(F, 3, 1, dtype=torch.float32, device=dev)
        dcb = torch.empty(F, dtype=torch.float32, device=dev)
    out = [None] * 6
    det = _hip_det.is_deterministic()
    with _on(dev):
        _check(lib.kge_convkb_score_triples_bwd(_p(E), E.stride(0), _p(R), R.stride(0), d, F, _p(ws), _p(h), _p(t), _p(r), B,
                                                _p(s), _p(go), _p(g), _p(rows), d, _p(dL), _p(dlb), _p(dw), _p(dcb),
                                                _stream()), 'kge_convkb_score_triples_bwd')
        for pos, n_rows, k0, k1, first in ((0, E.shape[0], h, t, 0), (1, R.shape[0], r, None, 2 * B)):
            if not needs[pos]:
                continue
            if row_grads:
                ids = r if k1 is None else torch.cat((k0, k1))
                out[pos] = sparse_rows(ids, rows[first:first + ids.shape[0]], (n_rows, d))
                continue
            grad = torch.zeros(n_rows, d, dtype=torch.float32, device=dev)
            if B:
                _hip_det.reduce_rows(rows[first:], d, d, k0, k1, grad, det=det)
            out[pos] = grad
    if want_par:
        for pos, val in ((2, dw), (3, dcb), (4, dL), (5, dlb)):
            out[pos] = val if needs[pos] else None
    return out
