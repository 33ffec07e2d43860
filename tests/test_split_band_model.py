# -*- coding: utf-8 -*-
"""CPU model check of the certified f16-split prefilter, independent of the GPU.

The count kernel decides `s_c >= s_true` from an f16 hi/lo-split MFMA accumulation and two thresholds per
query; the claim is:  acc >= a_hi  =>  the exact fp32 score counts,  acc < a_lo  =>  it does not.
Here the whole chain is restated in numpy -- the split (`split_rows_kernel`), the accumulation as
`tools/probe/mfma_probe.hip` measured it (per MFMA two passes of acc + 8 products, the 9 addends
truncated 24 bits below the largest, the sum exact, one round-to-nearest-even), the thresholds with the
prefix-norm magnitude bound (`split_thr_l2`, `split_acc_err`, `split_chain_err`) -- and the claim is
checked against the exact fp32 chain scores of the C oracle on adversarial inputs (near ties at every distance from the
threshold, exact duplicates, wide dynamic range, heavy cancellation), also with the band shrunk.  TEST INFRASTRUCTURE."""
import ctypes

import numpy as np
import pytest

from tests.helpers import oracle_clib, fptr
from tests.operand_ref import hi_lo

F = np.float32
S = F(4096.0)                       # SPLIT_SCALE_LOG2 = 12
TWO24, TWO22 = F(2.0 ** -24), F(2.0 ** -22)


def _split(x):
    """hi = f16(x * 2^12), lo = f16(x * 2^12 - hi)  (split_rows_kernel)."""
    hi, lo = hi_lo((x.astype(F) * S).astype(F))
    return hi.astype(np.float64), lo.astype(np.float64)


def _mfma_pass(acc, prods):
    """acc (P,) fp32 values as float64, prods (P, 8) exact products: one pass of the measured model."""
    add = np.concatenate([acc[:, None], prods], axis=1)
    mx = np.abs(add).max(axis=1)
    _, e = np.frexp(mx)                                   # mx = m * 2^e, m in [0.5, 1)  ->  exponent e - 1
    gran = np.ldexp(1.0, e - 1 - 24)
    gran[mx == 0] = 1.0
    tr = np.trunc(add / gran[:, None]) * gran[:, None]    # toward zero, 24 bits below the largest
    return tr.sum(axis=1).astype(F).astype(np.float64)    # exact sum (fits a double), one RNE rounding


def _split_accumulate(qh, ql, eh, el):
    """(B, N) accumulators of Sum_k qh*eh + qh*el + ql*eh, unit by unit, three MFMAs of two passes each."""
    B, Kp = qh.shape
    N = eh.shape[0]
    acc = np.zeros(B * N)
    for u in range(Kp // 16):
        for a, b in ((qh, eh), (qh, el), (ql, eh)):
            for half in range(2):
                sl = slice(u * 16 + half * 8, u * 16 + half * 8 + 8)
                prods = (a[:, None, sl] * b[None, :, sl]).reshape(B * N, 8)
                acc = _mfma_pass(acc, prods)
    return acc.reshape(B, N).astype(F)


def _thresholds(qn, st, em, K, units, amag, eps_scale, c_acc=F(1.25)):
    """split_thr_l2 with the prefix-norm magnitude sum (fp32 arithmetic as in the kernel)."""
    qn, st, amag = qn.astype(F), st.astype(F), amag.astype(F)
    eps_rel = F(3.01) * TWO22
    enrm, qnrm = np.sqrt(em) * F(1.000001), np.sqrt(qn) * F(1.000001)
    u = -st
    mag = qnrm * enrm + F(0.5) * em
    acc_err = c_acc * F(48.0) * TWO24 * (amag * F(1.003) + F(0.5) * em)
    chain_err = F(16.16) * TWO24 * amag * F(1.003)
    eps_dot = acc_err + chain_err + eps_rel * mag + F(2.5e-7) * (qnrm + enrm) + F(4e-9)
    eps_v = (F(2.0) * eps_dot + F(4.0) * TWO22 * (qn + em + np.abs(u))) * F(eps_scale)
    mid = F(0.5) * (qn - u)
    hw = F(0.5) * eps_v + TWO22 * (np.abs(qn) + np.abs(u))
    return ((mid - hw) * S * S).astype(F), ((mid + hw) * S * S).astype(F)


def _case(kind, B, N, K, rng):
    E = rng.standard_normal((N, K))
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    if kind == 'range':            # wide dynamic range inside every row
        E *= 10.0 ** rng.uniform(-3, 0, size=(N, K))
        E /= np.linalg.norm(E, axis=1, keepdims=True)
    R = rng.standard_normal((B, K)) * (0.6 / np.sqrt(K))
    h = rng.integers(0, N, B)
    Q = E[h] + R
    t = rng.integers(0, N, B)
    E = E.astype(F)
    if kind == 'ties':             # the true entity has exact duplicates and 1-ulp neighbours
        for i in range(B):
            c = rng.integers(0, N, 6)
            E[c[:3]] = E[t[i]]
            E[c[3:]] = np.nextafter(E[t[i]], F(np.inf) * np.sign(rng.standard_normal(K)).astype(F))
    if kind == 'near':             # candidates a relative 1e-7 .. 1e-4 away from the true entity: scores straddle the threshold
        free = [c for c in rng.permutation(N) if c not in set(t.tolist())]
        pos = 0
        for i in range(B):
            for s_ in (1e-7, 3e-7, 1e-6, 3e-6, 1e-5, 3e-5, 1e-4):
                for _ in range(3):
                    E[free[pos % len(free)]] = (E[t[i]].astype(np.float64) * (1 + s_ * rng.standard_normal(K))).astype(F)
                    pos += 1
    if kind == 'cancel':           # q almost orthogonal to most candidates: tiny dots out of large terms
        Q = np.where(np.arange(K)[None, :] % 2 == 0, 1.0, -1.0) * np.abs(Q) * 2.0
    return np.ascontiguousarray(Q.astype(F)), np.ascontiguousarray(E), t


@pytest.mark.parametrize('kind', ['plain', 'ties', 'near', 'range', 'cancel'])
@pytest.mark.parametrize('K', [200, 40, 512])
def test_split_band_is_certified_under_the_measured_accumulation_model(kind, K):
    lib = oracle_clib()
    rng = np.random.default_rng(hash((kind, K)) % 2 ** 32)
    B, N = 12, 300
    Q, E, t = _case(kind, B, N, K, rng)
    qn, en = np.empty(B, F), np.empty(N, F)
    lib.orc_row_sqnorm_chain(fptr(Q), ctypes.c_int64(K), ctypes.c_int64(B), ctypes.c_int64(K), fptr(qn))
    lib.orc_row_sqnorm_chain(fptr(E), ctypes.c_int64(K), ctypes.c_int64(N), ctypes.c_int64(K), fptr(en))
    exact = np.empty((B, N), F)
    i64 = ctypes.c_int64
    lib.orc_lp_gemm_chain(fptr(Q), i64(K), fptr(E), i64(K), i64(K), None, i64(0), None, i64(0), i64(0),
                          i64(B), i64(N), ctypes.c_int(1), fptr(qn), fptr(en), fptr(exact))
    st = exact[np.arange(B), t]
    assert float(qn.max() + en.max()) <= 16.0              # the evaluator's norm guard (fixed 2^12 scale)

    units = (K + 1 + 15) // 16
    Kp = units * 16
    Qa, Ea = np.zeros((B, Kp), F), np.zeros((N, Kp), F)
    Qa[:, :K], Ea[:, :K] = Q, E
    Qa[:, K] = 1.0                                         # queries carry 1, candidates -||e||^2 / 2
    Ea[:, K] = en * F(-0.5)
    qh, ql = _split(Qa)
    eh, el = _split(Ea)
    acc = _split_accumulate(qh, ql, eh, el)

    # prefix-norm magnitude sum (cell sums of the data columns, prefix maxima over the candidates)
    def cells(X):
        Xp = np.zeros((X.shape[0], Kp), np.float64)
        Xp[:, :K] = X
        return (Xp.reshape(X.shape[0], units, 16) ** 2).sum(axis=2)
    e2 = np.cumsum(cells(E), axis=1).max(axis=0)
    amag = np.sqrt(np.cumsum(cells(Q), axis=1) * e2[None, :]).sum(axis=1)
    em = F(en.max())

    counts_exact = exact >= st[:, None]
    for eps_scale in (1.0, 0.25):
        a_lo, a_hi = _thresholds(qn, st, em, K, units, amag, eps_scale)
        sure_yes, sure_no = acc >= a_hi[:, None], acc < a_lo[:, None]
        assert not (sure_yes & ~counts_exact).any(), (kind, K, eps_scale)
        assert not (sure_no & counts_exact).any(), (kind, K, eps_scale)
        uncertain = ~(sure_yes | sure_no)
        assert uncertain[np.arange(B), t].all() or kind == 'cancel'      # the true entity itself sits in the band
        assert uncertain.mean() < (0.3 if kind in ('ties', 'near', 'cancel') else 0.05)


# ---- the ONE-PRODUCT level (kge_split_args.level = 1, lp_split_common.h: split_thr_l2_hi; lp_split_mfma.hip: LV = 1 count kernel) ----------
def _hi_accumulate(qh, eh, units):
    """(B, N) accumulators of Sum_k qh*eh, one MFMA (two passes of 8 products) per k16 unit."""
    B, N = qh.shape[0], eh.shape[0]
    acc = np.zeros(B * N)
    for u in range(units):
        for half in range(2):
            sl = slice(u * 16 + half * 8, u * 16 + half * 8 + 8)
            acc = _mfma_pass(acc, (qh[:, None, sl] * eh[None, :, sl]).reshape(B * N, 8))
    return acc.reshape(B, N).astype(F)


def _thresholds_hi(qn, st, em, K, units, dq2, de2m, eps_scale, c_acc=F(1.25)):
    """split_thr_l2_hi (fp32 arithmetic as in the kernel): the band carries the measured residuals ||q - hi(q)||, max ||e - hi(e)||."""
    qn, st, dq2 = qn.astype(F), st.astype(F), dq2.astype(F)
    enrm, qnrm = np.sqrt(em) * F(1.000001), np.sqrt(qn) * F(1.000001)
    u = -st
    mag = qnrm * enrm + F(0.5) * em
    acc_err = c_acc * F(16.0) * TWO24 * (F(units) * mag)
    chain_err = F(1.01) * F(K) * TWO24 * mag
    dqn, den = np.sqrt(dq2) * F(1.0001), np.sqrt(F(de2m)) * F(1.0001)
    resid = (dqn * enrm + (qnrm + dqn) * den) * F(1.0005) + F(1.01) * TWO22 * F(0.5) * em
    eps_dot = acc_err + chain_err + resid + F(2.5e-7) * (qnrm + enrm) + F(4e-9)
    eps_v = (F(2.0) * eps_dot + F(4.0) * TWO22 * (qn + em + np.abs(u))) * F(eps_scale)
    mid = F(0.5) * (qn - u)
    hw = F(0.5) * eps_v + TWO22 * (np.abs(qn) + np.abs(u))
    return ((mid - hw) * S * S).astype(F), ((mid + hw) * S * S).astype(F)


@pytest.mark.parametrize('kind', ['plain', 'ties', 'near', 'range', 'cancel'])
@pytest.mark.parametrize('K', [200, 40, 512])
def test_one_product_band_is_certified_under_the_measured_accumulation_model(kind, K):
    """Level 1: acc = Sum_k hi(q) hi(e) + (1)(hi(aug)) + (1)(lo(aug)), one MFMA per unit; thresholds from the measured
    residuals.  acc >= a_hi => the exact score counts, acc < a_lo => it does not -- on the adversarial inputs of the
    three-product test; the band is wide (8x) but still a small fraction of the candidates."""
    lib = oracle_clib()
    rng = np.random.default_rng(1000 * K + ['plain', 'ties', 'near', 'range', 'cancel'].index(kind))
    B, N = 12, 300
    Q, E, t = _case(kind, B, N, K, rng)
    qn, en = np.empty(B, F), np.empty(N, F)
    i64 = ctypes.c_int64
    lib.orc_row_sqnorm_chain(fptr(Q), i64(K), i64(B), i64(K), fptr(qn))
    lib.orc_row_sqnorm_chain(fptr(E), i64(K), i64(N), i64(K), fptr(en))
    exact = np.empty((B, N), F)
    lib.orc_lp_gemm_chain(fptr(Q), i64(K), fptr(E), i64(K), i64(K), None, i64(0), None, i64(0), i64(0),
                          i64(B), i64(N), ctypes.c_int(1), fptr(qn), fptr(en), fptr(exact))
    st = exact[np.arange(B), t]
    units = (K + 2 + 15) // 16
    Kp = units * 16
    Qa, Ea = np.zeros((B, Kp), F), np.zeros((N, Kp), F)
    Qa[:, :K], Ea[:, :K] = Q, E
    qh = ((Qa * S).astype(F)).astype(np.float16).astype(np.float64)
    eh = ((Ea * S).astype(F)).astype(np.float16).astype(np.float64)
    # measured residuals (hi_rows_kernel / the query pipeline: exact fp32 differences, summed, unscaled)
    dq2 = ((((Qa * S).astype(F).astype(np.float64) - qh) ** 2).sum(axis=1) / float(S) ** 2 * 1.0001).astype(F)
    de2m = float(((((Ea * S).astype(F).astype(np.float64) - eh) ** 2).sum(axis=1) / float(S) ** 2 * 1.0001).max())
    # the two augmentation columns: queries 1, 1; candidates hi and lo of -||e||^2 / 2
    aug = (en * F(-0.5) * S).astype(F)
    a_hi_ = aug.astype(np.float16)
    a_lo_ = (aug - a_hi_.astype(F)).astype(F).astype(np.float16)
    qh[:, K] = qh[:, K + 1] = float(S)
    eh[:, K], eh[:, K + 1] = a_hi_.astype(np.float64), a_lo_.astype(np.float64)
    acc = _hi_accumulate(qh, eh, units)
    em = F(en.max())
    counts_exact = exact >= st[:, None]
    # (the residual term is a Cauchy-Schwarz bound on ACTUAL rounding errors -- tight for small K, where two residual
    # vectors can be nearly parallel: no large shrink factor survives; at K >= 200 half the band still certifies)
    for eps_scale in ((1.0, 0.5) if K >= 200 else (1.0,)):
        lo, hi = _thresholds_hi(qn, st, em, K, units, dq2, de2m, eps_scale)
        sure_yes, sure_no = acc >= hi[:, None], acc < lo[:, None]
        assert not (sure_yes & ~counts_exact).any(), (kind, K, eps_scale)
        assert not (sure_no & counts_exact).any(), (kind, K, eps_scale)
        uncertain = ~(sure_yes | sure_no)
        assert uncertain[np.arange(B), t].all() or kind == 'cancel'
        assert uncertain.mean() < (0.5 if kind in ('ties', 'near', 'cancel') else 0.2)


# ---- DOT mode on the one-product level with PER-QUERY operand scales (r05: kge_lp_dot_query_pipeline, split_thr_dot_hi) ------
def _split_scale(norm2):
    """split_scale of lp_split_common.h: the power of two that puts a row of squared norm `norm2` just inside f16 range."""
    m = np.sqrt(np.asarray(norm2, dtype=np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        e = np.floor(np.log2(16384.0 / m)) - 1.0
    e = np.clip(np.where(m > 0, e, 0.0), -100.0, 100.0)
    return np.where(m > 0, np.ldexp(1.0, e.astype(np.int64)), 1.0)


def _thresholds_dot_hi(qn, st, em, K, units, dq2, de2m, s_q, s_e, eps_scale, c_acc=F(1.25)):
    """split_thr_dot_hi (fp32 arithmetic as in the kernel): query i's thresholds carry ITS scale s_q[i] times the table's s_e."""
    qn, st, dq2 = qn.astype(F), st.astype(F), dq2.astype(F)
    enrm, qnrm = np.sqrt(F(em)) * F(1.000001), np.sqrt(qn) * F(1.000001)
    sqk = np.sqrt(F(K))
    eps_abs = F(1.4901161e-8) * sqk * (np.sqrt(qn) * enrm + np.sqrt(F(em)) * qnrm) + F(1e-30)
    acc_err = c_acc * F(16.0) * TWO24 * (F(units) * (qnrm * enrm))
    chain_err = F(1.01) * F(K) * TWO24 * (qnrm * enrm)
    dqn, den = np.sqrt(dq2) * F(1.0001), np.sqrt(F(de2m)) * F(1.0001)
    resid = (dqn * enrm + (qnrm + dqn) * den) * F(1.0005)
    eps_dot = (acc_err + chain_err + resid + eps_abs) * F(eps_scale)
    hw = eps_dot + TWO22 * np.abs(st)
    out_scale = (s_q * s_e).astype(F)
    return ((st - hw) * out_scale).astype(F), ((st + hw) * out_scale).astype(F)


@pytest.mark.parametrize('kind', ['plain', 'ties', 'near', 'range'])
@pytest.mark.parametrize('K', [200, 48, 400])
def test_dot_one_product_band_with_per_query_scales_is_certified(kind, K):
    """DistMult / ComplEx on level 1 as kge_lp_dot_query_pipeline prepares it: every QUERY row scaled by the power of two
    that fits its own norm (rows spread over four decades here -- a batch-wide scale would push the small rows into f16's
    subnormals), the candidate table by the one that fits its largest row; acc >= a_hi => the exact fp32 chain score
    counts, acc < a_lo => it does not; the guard column keeps a padding candidate (-65504 against the guard) below every
    threshold."""
    lib = oracle_clib()
    rng = np.random.default_rng(77 * K + ['plain', 'ties', 'near', 'range'].index(kind))
    B, N = 12, 300
    Q, E, t = _case(kind, B, N, K, rng)
    Q = (Q * (10.0 ** rng.uniform(-2, 2, size=(B, 1)))).astype(F)           # query rows of very different magnitude
    E = (E * (10.0 ** rng.uniform(-0.5, 0.5, size=(N, 1)))).astype(F)
    if kind in ('ties', 'near'):        # keep the duplicates / near-duplicates of the true entities what they were
        _, E0, _ = _case(kind, B, N, K, np.random.default_rng(77 * K + ['plain', 'ties', 'near', 'range'].index(kind)))
        E = (E0 * F(1.7)).astype(F)
    Q, E = np.ascontiguousarray(Q), np.ascontiguousarray(E)
    i64 = ctypes.c_int64
    exact = np.empty((B, N), F)
    lib.orc_lp_gemm_chain(fptr(Q), i64(K), fptr(E), i64(K), i64(K), None, i64(0), None, i64(0), i64(0),
                          i64(B), i64(N), ctypes.c_int(0), None, None, fptr(exact))
    st = exact[np.arange(B), t]
    qn = (Q.astype(np.float64) ** 2).sum(axis=1).astype(F)          # (a bound in this mode: any summation order)
    en = (E.astype(np.float64) ** 2).sum(axis=1).astype(F)
    em = F(en.max())
    s_q, s_e = _split_scale(qn), float(_split_scale(em))
    units = (K + 2 + 15) // 16
    Kp = units * 16
    Qa, Ea = np.zeros((B, Kp), np.float64), np.zeros((N + 1, Kp), np.float64)
    Qa[:, :K] = (Q.astype(np.float64) * s_q[:, None]).astype(F)      # (a power-of-two factor: the product is exact)
    Ea[:N, :K] = (E.astype(np.float64) * s_e).astype(F)
    qh, eh = Qa.astype(np.float16).astype(np.float64), Ea.astype(np.float16).astype(np.float64)
    assert np.isfinite(qh).all() and np.isfinite(eh).all()
    dq2 = (((Qa - qh)[:, :K] ** 2).sum(axis=1) / s_q ** 2 * 1.0001).astype(F)
    de2m = float((((Ea - eh)[:N, :K] ** 2).sum(axis=1) / s_e ** 2 * 1.0001).max())
    # the guard column: queries max(0.25 * ||q|| * (1 + 1/256) * s_q, 1), real candidates 0, the padding candidate -65504
    qr = np.sqrt(qn.astype(np.float64))
    qh[:, K] = np.maximum(0.25 * (qr + qr * 0.00390625) * s_q, 1.0).astype(F).astype(np.float16).astype(np.float64)
    eh[N, K] = -65504.0
    acc = _hi_accumulate(qh, eh, units)
    counts_exact = exact >= st[:, None]
    for eps_scale in ((1.0, 0.5) if K >= 200 else (1.0,)):
        lo, hi = _thresholds_dot_hi(qn, st, em, K, units, dq2, de2m, s_q, s_e, eps_scale)
        sure_yes, sure_no = acc[:, :N] >= hi[:, None], acc[:, :N] < lo[:, None]
        assert not (sure_yes & ~counts_exact).any(), (kind, K, eps_scale)
        assert not (sure_no & counts_exact).any(), (kind, K, eps_scale)
        assert (acc[:, N] < lo).all(), 'the padding candidate must stay below every threshold'
        uncertain = ~(sure_yes | sure_no)
        assert uncertain[np.arange(B), t].all()
        assert uncertain.mean() < 0.5
