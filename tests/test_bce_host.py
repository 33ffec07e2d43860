"""CPU-only tests of K-vs-all training: the float64 forms of tests/bce_ref.py against torch's own
binary_cross_entropy_with_logits, the exports / signatures / constants of include/kge_hip_bce.h, its workspace bound
(bounded over N: no (B, N) buffer), what the Python layer refuses, and the trainer's key batching."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import ROOT
from tests import bce_ref

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_bce, optim
from torchkge_amd.filter_index import FilterIndex, KEY2_SPAN
from torchkge_amd.utils import k_vs_all
from torchkge_amd.utils.training import KvsAllTrainer, OneVsAllTrainer

HEADER = os.path.join(ROOT, 'include', 'kge_hip_bce.h')
ENTRIES = ('kge_lp_bce_fwd', 'kge_lp_bce_bwd')
QUERIES = ('kge_lp_bce_ws_bytes', 'kge_lp_bce_chunks')


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def small_kg(n=23, n_ent=11, n_rel=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    h, t, r = (torch.randint(0, m, (n,), generator=g) for m in (n_ent, n_ent, n_rel))
    return tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                             rel2ix={i: i for i in range(n_rel)})


def random_csr(B, N, gen):
    """A CSR of B strictly ascending label sets of mixed length (empty ones included) in [0, N)."""
    sets = []
    for i in range(B):
        n = int(torch.randint(0, min(N, 9) + 1, (1,), generator=gen))
        sets.append(torch.randperm(N, generator=gen)[:n].sort().values)
    lens = torch.tensor([len(s) for s in sets])
    hi = torch.cumsum(lens, 0)
    return hi - lens, hi, (torch.cat(sets) if sets else torch.zeros(0)).to(torch.int32)


# ---------------------------------------------------------------------------
# the yardstick is torch's binary_cross_entropy_with_logits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_the_float64_forms_are_torch_bce_with_logits(eps):
    g = torch.Generator().manual_seed(3)
    for B, N, scale in ((1, 1, 1.0), (5, 2, 1.0), (37, 131, 3.0), (9, 300, 40.0)):
        S = (torch.randn(B, N, generator=g) * scale).double().requires_grad_()
        lo, hi, tg = random_csr(B, N, g)
        w = torch.rand(B, generator=g).double() + 0.5
        Y = bce_ref.dense_labels(lo, hi, tg, N)
        for i in range(B):
            assert Y[i].nonzero().view(-1).tolist() == tg[lo[i]:hi[i]].tolist()
        Ys = (1.0 - eps) * Y + eps / N
        rows = F.binary_cross_entropy_with_logits(S, Ys, reduction='none').sum(dim=1)
        (rows * w).sum().backward()
        assert torch.allclose(bce_ref.row_loss64(S, Y, eps), rows.detach(), rtol=1e-13, atol=1e-13), (B, N)
        G = bce_ref.g_matrix64(S, Y, eps, w)
        assert torch.allclose(G, S.grad, rtol=1e-12, atol=1e-15), (B, N)
        A, T = torch.randn(B, 7, generator=g).double(), torch.randn(N, 7, generator=g).double()
        dA, dT = bce_ref.grads64(S, Y, eps, w, A, T)
        assert torch.equal(dA, G @ T) and torch.equal(dT, G.t() @ A)
        # torch's 'mean' is the sum of the row sums over B * N
        mean = F.binary_cross_entropy_with_logits(S.detach(), Ys)
        assert torch.allclose(rows.detach().sum() / (B * N), mean, rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------
# the header and its binding
# ---------------------------------------------------------------------------
def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_bce.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(ENTRIES) | set(QUERIES)
    assert set(ENTRIES) == set(_hip_bce._SIGNATURES) and set(_hip_bce._WS_SIZES) == {QUERIES[0]}
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    from torchkge_amd.csrc import build as hb
    assert 'lp_bce.hip' in hb.SOURCES and hb.EXTRA_FLAGS['lp_bce.hip'] == hb._NO_SLP
    assert any(h.endswith('kge_hip_bce.h') for h in hb.HEADERS) and 'lp_tile64.h' in hb.HEADERS
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    # the sums' contract: no atomic in the source, nor in the skeleton it shares with the softmax criterion
    for name in ('lp_bce.hip', 'lp_tile64.h'):
        code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, name)).read())
        assert not re.search(r'atomic', code, flags=re.I), name
    hdr = open(HEADER).read()
    for name, value in (('KGE_BCE_BM', _hip_bce.BM), ('KGE_BCE_BN', _hip_bce.BN),
                        ('KGE_BCE_MIN_TILES_PER_CHUNK', _hip_bce.MIN_TILES_PER_CHUNK),
                        ('KGE_BCE_MAX_CHUNKS', _hip_bce.MAX_CHUNKS), ('KGE_BCE_MAX_K', _hip_bce.MAX_K),
                        ('KGE_BCE_KSLICE', _hip_bce.KSLICE)):
        m = re.search(r'#define %s (\d+)' % name, hdr)
        assert m and int(m.group(1)) == value, name


def test_one_score_tile_behind_both_criteria():
    """score_tile(), the two walks, the chunk arithmetic and the host half of the entries are defined once, in
    lp_tile64.h; both criteria include it, and neither includes the other's header."""
    from torchkge_amd.csrc import build as hb
    src = {n: open(os.path.join(hb.HERE, n)).read() for n in ('lp_tile64.h', 'lp_xent.hip', 'lp_bce.hip')}
    for fn in ('score_tile', 'grad_walk', 'sum_chunks'):
        assert len(re.findall(r'void %s\(' % fn, src['lp_tile64.h'])) == 1
        for n in ('lp_xent.hip', 'lp_bce.hip'):
            assert not re.search(r'void %s\(' % fn, src[n]), (fn, n)
    for fn in ('void stats_walk', 'void chunk_tiles', 'int chunk_count', 'int setup', 'int launch_fwd', 'int launch_bwd'):
        assert len(re.findall(r'\b%s\(' % fn, src['lp_tile64.h'])) == 1, fn
        for n in ('lp_xent.hip', 'lp_bce.hip'):
            assert not re.search(r'\b%s\(' % fn, src[n]), (fn, n)
    for n in ('lp_xent.hip', 'lp_bce.hip'):
        code = re.sub(r'//[^\n]*', '', src[n])
        assert '#include "lp_tile64.h"' in src[n] and 'mfma' not in code.lower()
        # the chunk partition is written in the skeleton alone, and the skeleton's users all go through chunk_tiles()
        assert not re.search(r'col_tiles\s*\*', code) and 'hipLaunchKernelGGL' not in code, n
    assert len(re.findall(r'col_tiles\s*\*', re.sub(r'//[^\n]*', '', src['lp_tile64.h']))) == 2      # t0 and t1, once
    assert 'kge_hip_xent.h' not in src['lp_bce.hip'] and 'kge_hip_bce.h' not in src['lp_xent.hip']
    assert 'kge_hip_xent.h' not in src['lp_tile64.h'] and 'kge_hip_bce.h' not in src['lp_tile64.h']


def test_ctypes_signatures_match_the_header_prototypes():
    protos = dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', header_text(), flags=re.S))

    def kind(param):
        param = param.strip()
        if '*' in param:
            return ctypes.c_void_p
        t = param.split()
        for word, c in (('kge_stream_t', ctypes.c_void_p), ('int64_t', ctypes.c_int64), ('size_t', ctypes.c_size_t),
                        ('float', ctypes.c_float), ('int', ctypes.c_int)):
            if word in t:
                return c
        raise AssertionError('unparsed parameter: %r' % param)
    assert set(protos) == set(ENTRIES) | {'kge_lp_bce_chunks'}
    lib = _hip_bce.load_library()
    for name, args in _hip_bce._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            assert a is kind(prm), (name, prm)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    f = lib.kge_lp_bce_ws_bytes
    assert f.argtypes == [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int] and f.restype is ctypes.c_size_t
    assert re.search(r'\bsize_t\s+kge_lp_bce_ws_bytes\s*\(\s*int64_t \w+,\s*int64_t \w+,\s*int \w+,\s*int \w+\s*\)\s*;',
                     open(HEADER).read())
    assert [kind(p) for p in protos['kge_lp_bce_chunks'].split(',')] == [ctypes.c_int64]
    assert lib.kge_lp_bce_chunks.argtypes == [ctypes.c_int64] and lib.kge_lp_bce_chunks.restype is ctypes.c_int


def test_the_main_header_does_not_know_the_entries():
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    for name in ENTRIES + QUERIES:
        assert name.encode() not in raw
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


# ---------------------------------------------------------------------------
# geometry and workspace (host arithmetic: a process without a GPU)
# ---------------------------------------------------------------------------
def test_chunks_is_a_capped_function_of_n():
    BN, MT, CAP = _hip_bce.BN, _hip_bce.MIN_TILES_PER_CHUNK, _hip_bce.MAX_CHUNKS
    assert [_hip_bce.chunks(n) for n in (-3, 0)] == [0, 0]
    assert [_hip_bce.chunks(n) for n in (1, 2, BN, BN + 1, MT * BN)] == [1] * 5
    assert _hip_bce.chunks(MT * BN + 1) == 2 and _hip_bce.chunks(2 * MT * BN) == 2 and _hip_bce.chunks(2 * MT * BN + 1) == 3
    for n in [1, 63, 64, 65, 257, 1000, 14951, 40943, 10 ** 6, 1 << 20, 1 << 24, (1 << 31) - 1]:
        assert _hip_bce.chunks(n) == min(CAP, -(-(-(-n // BN)) // MT)), n
    assert _hip_bce.chunks(MT * BN * (CAP - 1) + 1) == CAP == _hip_bce.chunks(1 << 30)


def test_workspace_is_bounded_over_n_and_monotone_in_b():
    f = _hip_bce.load_library().kge_lp_bce_ws_bytes
    for B, N, K0, K1 in ((0, 10, 4, 0), (-1, 10, 4, 0), (5, 0, 4, 0), (5, -2, 4, 0), (5, 10, 0, 0), (5, 10, 4, -1),
                         (5, 10, 1025, 0), (5, 10, 513, 512), (1 << 31, 10, 4, 0), (5, 1 << 31, 4, 0)):
        assert int(f(B, N, K0, K1)) == 0, (B, N, K0, K1)
    assert int(f(5, 10, 1024, 0)) > 0 and int(f(5, 10, 512, 512)) > 0
    # monotone in B, the documented formula: three fp64 partials per (row, chunk) and the partial dA panels
    for N, K0, K1 in ((1, 1, 0), (300, 20, 0), (14951, 200, 0), (1 << 20, 512, 512)):
        prev = 0
        c = _hip_bce.chunks(N)
        for B in (1, 2, 63, 64, 65, 133, 2048):
            b = int(f(B, N, K0, K1))
            assert b > prev and b % 4 == 0, (B, N)
            assert b == 24 * B * c + 4 * c * B * (K0 + K1)
            prev = b
    # constant in N beyond the chunk cap, far below one (B, N) fp32 matrix
    cap_n = _hip_bce.BN * _hip_bce.MIN_TILES_PER_CHUNK * (_hip_bce.MAX_CHUNKS - 1) + 1
    for B, K0, K1 in ((1, 8, 0), (2048, 200, 0), (2048, 512, 512)):
        a, b = int(f(B, 1 << 20, K0, K1)), int(f(B, 1 << 24, K0, K1))
        assert a == b > 0
        assert a < 4 * B * (1 << 20)
        assert a == int(f(B, (1 << 31) - 1, K0, K1)) == int(f(B, cap_n, K0, K1)) > int(f(B, cap_n - 1, K0, K1))
    assert int(f(1024, 10 ** 6, 512, 512)) == 24 * 1024 * 32 + 4 * 32 * 1024 * 1024      # the 0.13 GB of the 1e6 step
    assert _hip_bce.ws_bytes(70, 300, 20) == int(f(70, 300, 20, 0)) and (70, 300, 20, 0) in _hip_bce._WS_BYTES


# ---------------------------------------------------------------------------
# what the Python layer refuses
# ---------------------------------------------------------------------------
def host_labels(B):
    z = torch.zeros(B, dtype=torch.long)
    return z, z, torch.zeros(1, dtype=torch.int32)


def test_host_tensors_are_refused_before_any_launch():
    Q, E, lab = torch.zeros(3, 4), torch.zeros(5, 4), host_labels(3)
    with pytest.raises(RuntimeError, match='MI355X'):
        k_vs_all.all_candidates_bce(Q, E, lab)
    with pytest.raises(RuntimeError, match='MI355X'):
        k_vs_all.all_candidates_bce((Q, Q), (E, E), lab, label_smoothing=0.1, reduction='sum')
    e = torch.zeros(3, dtype=torch.long)
    for model in (tk.DistMultModel(4, 11, 3), tk.ComplExModel(4, 11, 3)):
        for side in ('tail', 'head'):
            with pytest.raises(RuntimeError, match='MI355X'):
                model.k_vs_all_loss(e, e, lab, side)


def test_bad_arguments_raise_value_errors():
    Q, E, lab = torch.zeros(3, 4), torch.zeros(5, 4), host_labels(3)
    with pytest.raises(ValueError, match='reduction'):
        k_vs_all.all_candidates_bce(Q, E, lab, reduction='batchmean')
    for eps in (-0.1, 1.5):
        with pytest.raises(ValueError, match='label_smoothing'):
            k_vs_all.all_candidates_bce(Q, E, lab, label_smoothing=eps)
    for bad in (lab[:2], lab[0], None):
        with pytest.raises(ValueError, match='seg_lo, seg_hi, targets'):
            k_vs_all.all_candidates_bce(Q, E, bad)
    e = torch.zeros(3, dtype=torch.long)
    for model in (tk.DistMultModel(4, 11, 3), tk.ComplExModel(4, 11, 3)):
        for side in ('both', 'tails', None):
            with pytest.raises(ValueError, match="'tail' or 'head'"):
                model.k_vs_all_loss(e, e, lab, side)
    kg = small_kg()
    model = tk.DistMultModel(4, 11, 3)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    with pytest.raises(ValueError, match="'both', 'tail' or 'head'"):
        KvsAllTrainer(model, kg, 2, 5, opt, side='left')
    for use_cuda in (None, 'cpu'):
        with pytest.raises(ValueError, match='live on the GPU'):
            KvsAllTrainer(model, kg, 2, 5, opt, use_cuda=use_cuda)


def test_models_without_the_criterion_name_the_two_that_have_it():
    e, lab = torch.zeros(3, dtype=torch.long), host_labels(3)
    kg = small_kg()
    others = [tk.TransEModel(4, 11, 3, 'L2'), tk.TransHModel(4, 11, 3), tk.RESCALModel(4, 11, 3), tk.HolEModel(4, 11, 3),
              tk.AnalogyModel(4, 11, 3)]
    for model in others:
        with pytest.raises(NotImplementedError, match='DistMultModel and ComplExModel') as err:
            model.k_vs_all_loss(e, e, lab, 'tail')
        assert type(model).__name__ in str(err.value) and 'k_vs_all_loss' in str(err.value)
        with pytest.raises(NotImplementedError, match='DistMultModel and ComplExModel'):
            KvsAllTrainer(model, kg, 2, 5, torch.optim.SGD(model.parameters(), lr=0.1))


def test_row_optimizers_are_refused_and_the_trainer_keeps_its_arguments():
    kg = small_kg()
    model = tk.ComplExModel(4, 11, 3)
    for cls in (optim.RowSGD, optim.RowAdagrad, optim.RowAdam):
        with pytest.raises(ValueError, match='dense') as e:
            KvsAllTrainer(model, kg, 2, 5, cls(model.parameters(), lr=0.1))
        assert cls.__name__ in str(e.value) and 'torch.optim' in str(e.value)
    opt = torch.optim.Adagrad(model.parameters(), lr=0.1)
    tr = KvsAllTrainer(model, kg, 2, 5, opt, 0.1, 'tail', verbose=False)
    assert (tr.n_epochs, tr.batch_size, tr.label_smoothing, tr.side, tr.use_cuda, tr.n_triples) == (2, 5, 0.1, 'tail', 'all', 23)
    assert tr.epoch_losses == [] and tr.sync_free is False and tr.optimizer is opt
    d = KvsAllTrainer(model, kg, 2, 5, opt)
    assert (d.label_smoothing, d.side, d.use_cuda) == (0.0, 'both', 'all')
    # the 1-vs-all trainer is as it was
    import inspect
    assert list(inspect.signature(OneVsAllTrainer.__init__).parameters) == list(inspect.signature(KvsAllTrainer.__init__).parameters)


# ---------------------------------------------------------------------------
# the trainer's key batching: pure index arithmetic
# ---------------------------------------------------------------------------
def test_key_batches_cover_every_distinct_key_once_with_its_answers():
    # a hand-made graph: a hub key (0, 0) with seven tails, duplicate facts, a key that exists on one side only
    facts = [(0, 0, t) for t in (9, 1, 4, 10, 2, 7, 3)] + [(0, 0, 4), (1, 0, 4), (1, 1, 4), (5, 2, 5), (5, 2, 5), (6, 1, 0),
                                                          (10, 2, 10), (3, 0, 9), (3, 1, 9), (2, 2, 0)]
    h, r, t = (torch.tensor(x) for x in zip(*facts))
    tails, heads = {}, {}
    for a, b, c in facts:
        tails.setdefault((a, b), set()).add(c)
        heads.setdefault((c, b), set()).add(a)
    for key1, values, expect in ((h, t, tails), (t, h, heads)):
        index = FilterIndex.from_triples_torch(key1, r, values, 'cpu', 11, 3, 11)
        assert index.n_keys == len(expect)
        for batch_size in (1, 4, 5, len(expect), len(expect) + 3):
            seen = []
            sizes = []
            for e, rel, lo, hi in KvsAllTrainer.key_batches(index, batch_size):
                assert e.shape == rel.shape == lo.shape == hi.shape and e.dtype == torch.int64
                sizes.append(e.shape[0])
                for j in range(e.shape[0]):
                    key = (int(e[j]), int(rel[j]))
                    seg = index.targets[int(lo[j]):int(hi[j])].tolist()
                    assert seg == sorted(expect[key]), key        # sorted, duplicate-free, the key's whole answer set
                    assert int(e[j]) * KEY2_SPAN + int(rel[j]) == int(index.keys[len(seen)])      # index order
                    seen.append(key)
            assert len(seen) == len(set(seen)) == len(expect) and set(seen) == set(expect)
            assert all(s == batch_size for s in sizes[:-1]) and 0 < sizes[-1] <= batch_size
            assert len(sizes) == -(-len(expect) // batch_size)
