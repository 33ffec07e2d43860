"""CPU-only tests of the grouped scorer (include/kge_hip_factgroup.h): the exports and ctypes signatures, the
KGE_EINVAL / KGE_EUNSUPPORTED table of both entries on never-dereferenced aligned addresses (every refusal happens before
a launch), the host arithmetic (rows per fact of a kind, rows, bytes and ids of a batch), a pure-Python restatement of
the contract (which negative counts as head-corrupted, the id vector, the rows buffer's blocks), and the unchanged
leading parameters of Trainer."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from tests.helpers import ROOT

from torchkge_amd import _hip, _hip_factgroup as fg
from torchkge_amd.utils.training import Trainer

HEADER = os.path.join(ROOT, 'include', 'kge_hip_factgroup.h')
ENTRIES = ('kge_score_fact_groups', 'kge_score_fact_groups_bwd')
QUERIES = ('kge_fact_group_forward_chunks', 'kge_fact_group_entity_tables', 'kge_fact_group_relation_tables', 'kge_fact_group_rows_per_fact',
           'kge_fact_group_rows', 'kge_fact_group_rows_bytes', 'kge_fact_group_ids')
EINVAL, EUNSUPPORTED = -1, -3
TEN = sorted(fg.KINDS)
OTHERS = [_hip.RESCAL, _hip.HOLE, _hip.TRANSR, -1, 13, 99]
# (entity tables, relation tables) per kind
SHAPE = {k: (1, 1) for k in TEN}
SHAPE.update({_hip.TRANSH: (1, 2), _hip.COMPLEX: (2, 2), _hip.TRANSD: (2, 2)})


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_library_exports_every_symbol_the_header_declares_and_the_build_lists_the_file():
    lib = fg.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(ENTRIES) | set(QUERIES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    for name in declared:
        assert hasattr(lib, name), name
    from torchkge_amd.csrc import build as hb
    assert 'score_fact_groups.hip' in hb.SOURCES and 'score_fact_groups.hip' not in hb.EXTRA_FLAGS
    assert 'score_triples.hip' not in hb.EXTRA_FLAGS            # the same flags: the bit-equality depends on it
    assert 'score_rows.h' in hb.HEADERS and any(h.endswith('kge_hip_factgroup.h') for h in hb.HEADERS)
    for name in ('score_fact_groups.hip', 'score_triples.hip'):
        assert '#include "score_rows.h"' in open(os.path.join(hb.HERE, name)).read(), name
    # row mode only: no atomic in the new translation unit
    code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, 'score_fact_groups.hip')).read())
    assert not re.search(r'atomic', code, flags=re.I)
    for name, value in (('WAVES', fg.WAVES), ('K_PER_CHUNK', fg.K_PER_CHUNK), ('MAX_CHUNKS', fg.MAX_CHUNKS)):
        m = re.search(r'#define KGE_FACT_GROUP_%s (\d+)' % name, open(HEADER).read())
        assert m and int(m.group(1)) == value, name
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    for name in ENTRIES + QUERIES:
        assert name.encode() not in raw and name not in _hip._SIGNATURES
    assert _hip.ABI_VERSION == 33 and int(lib.kge_abi_version()) == 33


def test_ctypes_signatures_match_the_header_prototypes():
    protos = dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', header_text(), flags=re.S))

    def kind(param):
        t = param.strip().split()
        if '*' in param or 'kge_stream_t' in t:
            return ctypes.c_void_p
        if 'int64_t' in t:
            return ctypes.c_int64
        if 'int' in t:
            return ctypes.c_int
        raise AssertionError('unparsed parameter: %r' % param)
    assert set(protos) == set(fg._SIGNATURES)
    lib = fg.load_library()
    for name, args in fg._SIGNATURES.items():
        params = protos[name].split(',')
        assert [kind(p) for p in params] == args, name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    i64, i32 = ctypes.c_int64, ctypes.c_int
    for name, args, res in (('kge_fact_group_rows_per_fact', [i32, i64], i64), ('kge_fact_group_rows', [i32, i64, i64], i64),
                            ('kge_fact_group_rows_bytes', [i32, i64, i64, i64], ctypes.c_size_t),
                            ('kge_fact_group_ids', [i64, i64], i64)):
        f = getattr(lib, name)
        assert f.argtypes == args and f.restype is res, name
        ret = 'size_t' if res is ctypes.c_size_t else 'int64_t'
        assert re.search(r'\b%s\s+%s\s*\(' % (ret, name), header_text()), name


# ---------------------------------------------------------------------------
# the refusals: every one before a launch, on addresses nobody reads
# ---------------------------------------------------------------------------
A = [4096 * (i + 1) for i in range(16)]     # 16-byte aligned, never dereferenced


def fwd(lib, kind, d_ent=8, d_rel=8, B=4, K=3, tabs=None, h=A[4], t=A[5], r=A[6], nh=A[7], nt=A[8], pos=A[9], neg=A[10], ld=None):
    tabs = A[:4] if tabs is None else tabs
    return int(lib.kge_score_fact_groups(kind, tabs[0], tabs[1], tabs[2], tabs[3], d_ent, d_rel, h, t, r, B, nh, nt, K, pos, neg,
                                         B if ld is None else ld, None))


def bwd(lib, kind, d_ent=8, d_rel=8, B=4, K=3, tabs=None, h=A[4], t=A[5], r=A[6], nh=A[7], nt=A[8], gp=A[9], gn=A[10], ld=None,
        rows=A[11], rows_ld=None, ids=A[12]):
    tabs = A[:4] if tabs is None else tabs
    return int(lib.kge_score_fact_groups_bwd(kind, tabs[0], tabs[1], tabs[2], tabs[3], d_ent, d_rel, h, t, r, B, nh, nt, K, gp, gn,
                                             B if ld is None else ld, rows, d_ent if rows_ld is None else rows_ld, ids, None))


@pytest.mark.parametrize('entry', [fwd, bwd])
def test_argument_checks_return_einval_before_any_launch(entry):
    lib = fg.load_library()
    for kind in OTHERS:
        assert entry(lib, kind) == EINVAL, kind
    for kind in TEN:
        assert entry(lib, kind, K=0) == EINVAL and entry(lib, kind, K=-2) == EINVAL, kind
        assert entry(lib, kind, B=-1) == EINVAL, kind
        assert entry(lib, kind, B=1 << 16, K=1 << 15) == EINVAL, kind      # B * K = 2^31
        assert entry(lib, kind, B=(1 << 31) - 1, K=2) == EINVAL, kind
        assert entry(lib, kind, ld=3) == EINVAL, kind                       # ld < B
        for name in ('h', 't', 'r', 'nh', 'nt'):
            assert entry(lib, kind, **{name: None}) == EINVAL, (kind, name)
        assert entry(lib, kind, tabs=[None, A[1], A[2], A[3]]) == EINVAL and entry(lib, kind, tabs=[A[0], None, A[2], A[3]]) == EINVAL
        n_tab = sum(SHAPE[kind]) if kind != _hip.TRANSH else 3
        if n_tab >= 3:
            assert entry(lib, kind, tabs=[A[0], A[1], None, A[3]]) == EINVAL, kind
        if n_tab == 4:
            assert entry(lib, kind, tabs=[A[0], A[1], A[2], None]) == EINVAL, kind
        assert entry(lib, kind, d_ent=0, d_rel=0) == EINVAL and entry(lib, kind, d_ent=-4, d_rel=-4) == EINVAL, kind
        if kind == _hip.TRANSD:
            assert entry(lib, kind, d_ent=8, d_rel=12) == EINVAL            # d_rel <= d_ent
        else:
            assert entry(lib, kind, d_ent=8, d_rel=4) == EINVAL, kind       # one width
        for d in (1025, 1028, 4096):                                        # beyond the register-resident kernels
            assert entry(lib, kind, d_ent=d, d_rel=d) == EINVAL, (kind, d)
        # B = 0 launches nothing and looks at no pointer behind the tables
        assert entry(lib, kind, B=0, K=0, h=None, t=None, r=None, nh=None, nt=None) == 0, kind
    for kind in TEN:
        assert fwd(lib, kind, pos=None) == EINVAL and fwd(lib, kind, neg=None) == EINVAL
        for name in ('gp', 'gn', 'rows', 'ids'):
            assert bwd(lib, kind, **{name: None}) == EINVAL, (kind, name)
        assert bwd(lib, kind, rows_ld=7) == EINVAL                          # rows_ld < d_ent


@pytest.mark.parametrize('entry', [fwd, bwd])
def test_the_sixteen_register_bucket_is_refused_as_unsupported(entry):
    """Rows of 513 .. 1024 floats: valid arguments, nothing launched, KGE_EUNSUPPORTED -- on the 16-byte path (516, 1024)
    and on the scalar one (513, 1023; tables off a 16-byte boundary)."""
    lib = fg.load_library()
    for kind in TEN:
        for d in (513, 516, 1023, 1024):
            assert entry(lib, kind, d_ent=d, d_rel=d) == EUNSUPPORTED, (kind, d)
        assert entry(lib, kind, d_ent=516, d_rel=516, tabs=[a + 4 for a in A[:4]]) == EUNSUPPORTED, kind
        assert entry(lib, kind, d_ent=516, d_rel=516, K=0) == EINVAL, kind  # the argument checks come first
    assert entry(lib, _hip.TRANSD, d_ent=600, d_rel=8) == EUNSUPPORTED      # the entity rows set the bucket


# ---------------------------------------------------------------------------
# host arithmetic
# ---------------------------------------------------------------------------
def test_rows_per_fact_per_kind():
    lib = fg.load_library()
    for kind in TEN:
        e, q = SHAPE[kind]
        assert (int(lib.kge_fact_group_entity_tables(kind)), int(lib.kge_fact_group_relation_tables(kind))) == (e, q)
        assert tuple(len(x) for x in fg.tables_of(kind)) == (e, q)
        for K in (1, 2, 5, 256, 1024):
            assert fg.rows_per_fact(kind, K) == e * (K + 2) + q, (kind, K)
        assert fg.rows_per_fact(kind, 0) == 0 and fg.rows_per_fact(kind, -3) == 0
    # the issue's numbers: K + 3, K + 4, 2 K + 6, against 3 (K + 1), 4 (K + 1), 6 (K + 1) of kge_score_triples_bwd
    K = 256
    assert fg.rows_per_fact(_hip.TRANSE_L2, K) == 259 < 3 * (K + 1) == 771
    assert fg.rows_per_fact(_hip.DISTMULT, K) == fg.rows_per_fact(_hip.TORUSE_TORUS_L2, K) == K + 3
    assert fg.rows_per_fact(_hip.TRANSH, K) == K + 4
    assert fg.rows_per_fact(_hip.COMPLEX, K) == fg.rows_per_fact(_hip.TRANSD, K) == 2 * K + 6
    for kind in OTHERS:
        assert fg.rows_per_fact(kind, 4) == 0
        assert int(lib.kge_fact_group_entity_tables(kind)) == 0 and int(lib.kge_fact_group_relation_tables(kind)) == 0
    # the tables of a block are those kge_score_triples_bwd's streams name for the same ids
    for kind in TEN:
        ent, rel = fg.tables_of(kind)
        assert [ti for ti, s0, ns, key in _hip._BWD_STREAMS[kind] if key == 'ht'] == list(ent)
        assert [ti for ti, s0, ns, key in _hip._BWD_STREAMS[kind] if key == 'r'] == list(rel)


def test_rows_bytes_and_ids_are_monotone_and_zero_for_empty_batches():
    lib = fg.load_library()
    for kind in TEN:
        for B in (0, -1, -100):
            assert int(lib.kge_fact_group_rows(kind, B, 4)) == 0 and int(lib.kge_fact_group_rows_bytes(kind, B, 4, 8)) == 0
            assert int(lib.kge_fact_group_ids(B, 4)) == 0
        assert int(lib.kge_fact_group_rows(kind, 4, 0)) == 0 and int(lib.kge_fact_group_ids(4, 0)) == 0
        assert int(lib.kge_fact_group_rows(kind, 1 << 16, 1 << 15)) == 0    # B * K >= 2^31
        assert int(lib.kge_fact_group_rows_bytes(kind, 4, 4, 0)) == 0
        last = 0
        for B, K, ld in ((1, 1, 1), (1, 1, 8), (1, 2, 8), (2, 2, 8), (7, 5, 8), (7, 5, 12), (300, 67, 200), (512, 1024, 200),
                         (512, 1024, 512), (1024, 1024, 512)):
            rows, nb = int(lib.kge_fact_group_rows(kind, B, K)), int(lib.kge_fact_group_rows_bytes(kind, B, K, ld))
            assert rows == B * fg.rows_per_fact(kind, K) and nb == rows * ld * 4, (kind, B, K, ld)
            assert nb > last, (kind, B, K, ld)
            last = nb
            assert int(lib.kge_fact_group_ids(B, K)) == B * (K + 2)
    for kind in OTHERS:
        assert int(lib.kge_fact_group_rows(kind, 4, 4)) == 0 and int(lib.kge_fact_group_rows_bytes(kind, 4, 4, 8)) == 0


# ---------------------------------------------------------------------------
# the contract, restated
# ---------------------------------------------------------------------------
def contract(h, t, neg_h, neg_t):
    """(head-corrupted?, replaced entity, the negative's (head, tail)) per negative, and the id vector, in pure Python."""
    B, K = len(h), len(neg_h) // len(h)
    head, repl, triple = [], [], []
    for k in range(K):
        for i in range(B):
            at = k * B + i
            hc = neg_h[at] != h[i]
            head.append(hc)
            repl.append(neg_h[at] if hc else neg_t[at])
            triple.append((neg_h[at], t[i]) if hc else (h[i], neg_t[at]))
    return head, repl, triple, list(h) + list(t) + repl


def test_contract_restatement_head_corruption_and_the_id_vector():
    h, t = [3, 5, 5, 0], [4, 5, 1, 0]
    #            k = 0: head, tail, tail == t (legal), tail      k = 1: head == t side value, tail, both (broken), head
    neg_h = [9, 5, 5, 0] + [4, 5, 8, 7]
    neg_t = [4, 2, 1, 6] + [4, 5, 9, 0]
    head, repl, triple, ids = contract(h, t, neg_h, neg_t)
    assert head == [True, False, False, False, True, False, True, True]
    assert repl == [9, 2, 1, 6, 4, 5, 8, 7]
    # a negative inside the contract is its own (neg_h, neg_t); the broken one (k = 1, i = 2) is (neg_h, t[i])
    for at, (hc, tr) in enumerate(zip(head, triple)):
        i = at % 4
        if not (neg_h[at] != h[i] and neg_t[at] != t[i]):
            assert tr == (neg_h[at], neg_t[at]), at
    assert triple[6] == (8, 1) and neg_t[6] == 9
    assert ids == h + t + repl and len(ids) == 4 * (2 + 2)
    # the blocks of the rows buffer: entity table s from row s (K + 2) B, relation table q behind the entity tables
    B, K = 4, 2
    for kind in TEN:
        e, q = SHAPE[kind]
        starts = [s * (K + 2) * B for s in range(e)] + [e * (K + 2) * B + j * B for j in range(q)]
        sizes = [(K + 2) * B] * e + [B] * q
        assert starts[-1] + sizes[-1] == B * fg.rows_per_fact(kind, K)
        assert all(a + n == b for a, n, b in zip(starts, sizes, starts[1:]))       # adjacent: each block is one view
    # the slices of the K negatives over the wavefronts of a block cover [0, K) in order, some empty below WAVES
    lib = fg.load_library()
    for K in (1, 2, 3, 4, 5, 67, 128, 129, 300, 1024, 128 * 1024, 128 * 1024 + 1, 10 ** 7):
        cuts = [w * K // fg.WAVES for w in range(fg.WAVES + 1)]
        assert cuts[0] == 0 and cuts[-1] == K and cuts == sorted(cuts)
        assert (K < fg.WAVES) == any(a == b for a, b in zip(cuts, cuts[1:]))
        # the forward: chunks first (never empty), then the wavefronts' slices of every chunk
        C = int(lib.kge_fact_group_forward_chunks(K))
        assert C == min(-(-K // fg.K_PER_CHUNK), fg.MAX_CHUNKS) >= 1
        chunks = [c * K // C for c in range(C + 1)]
        assert chunks[0] == 0 and chunks[-1] == K and all(a < b for a, b in zip(chunks, chunks[1:]))
        seen = 0
        for k0, k1 in list(zip(chunks, chunks[1:]))[:3] + list(zip(chunks, chunks[1:]))[-3:]:
            sl = [k0 + w * (k1 - k0) // fg.WAVES for w in range(fg.WAVES + 1)]
            assert sl[0] == k0 and sl[-1] == k1 and sl == sorted(sl)
            seen += 1
        assert seen
    assert int(lib.kge_fact_group_forward_chunks(0)) == 0 and int(lib.kge_fact_group_forward_chunks(-5)) == 0


def test_trainer_switch_is_off_by_default_and_the_constructor_is_unchanged():
    sig = inspect.signature(Trainer.__init__)
    assert list(sig.parameters)[-5:] == ['fused', 'sync_free', 'sampler', 'verbose', 'n_neg']
    assert Trainer.grouped_forward is False and 'grouped_forward' not in sig.parameters
    from torchkge_amd.models.interfaces import Model
    fsig = inspect.signature(Model.forward_grouped)
    assert list(fsig.parameters)[:6] == ['self', 'heads', 'tails', 'relations', 'negative_heads', 'negative_tails']
    assert fsig.parameters['check'].kind is inspect.Parameter.KEYWORD_ONLY and fsig.parameters['check'].default is True
