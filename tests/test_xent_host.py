"""CPU-only tests of 1-vs-all training: the float64 forms of tests/xent_ref.py against torch's own cross_entropy, the
exports / signatures / constants of include/kge_hip_xent.h, its workspace bound (bounded over N: no (B, N) buffer), and
what the Python layer refuses."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import ROOT
from tests import xent_ref

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_xent, optim
from torchkge_amd.utils import one_vs_all
from torchkge_amd.utils.training import OneVsAllTrainer, Trainer

HEADER = os.path.join(ROOT, 'include', 'kge_hip_xent.h')
ENTRIES = ('kge_lp_xent_fwd', 'kge_lp_xent_bwd')
QUERIES = ('kge_lp_xent_ws_bytes', 'kge_lp_xent_chunks')


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def small_kg(n=23, n_ent=11, n_rel=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    h, t, r = (torch.randint(0, m, (n,), generator=g) for m in (n_ent, n_ent, n_rel))
    return tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                             rel2ix={i: i for i in range(n_rel)})


# ---------------------------------------------------------------------------
# the yardstick is torch's cross_entropy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_the_float64_forms_are_torch_cross_entropy(eps):
    g = torch.Generator().manual_seed(3)
    for B, N, scale in ((1, 1, 1.0), (5, 2, 1.0), (37, 131, 3.0), (9, 300, 40.0)):
        S = (torch.randn(B, N, generator=g) * scale).double().requires_grad_()
        t = torch.randint(0, N, (B,), generator=g)
        w = torch.rand(B, generator=g).double() + 0.5
        rows = F.cross_entropy(S, t, label_smoothing=eps, reduction='none')
        (rows * w).sum().backward()
        lse, loss = xent_ref.row_loss64(S, t, eps)
        assert torch.allclose(lse, torch.logsumexp(S.detach(), dim=1), rtol=1e-14, atol=1e-14)
        assert torch.allclose(loss, rows.detach(), rtol=1e-13, atol=1e-13), (B, N)
        G = xent_ref.g_matrix64(S, t, eps, w)
        assert torch.allclose(G, S.grad, rtol=1e-12, atol=1e-15), (B, N)
        A, T = torch.randn(B, 7, generator=g).double(), torch.randn(N, 7, generator=g).double()
        dA, dT = xent_ref.grads64(S, t, eps, w, A, T)
        assert torch.equal(dA, G @ T) and torch.equal(dT, G.t() @ A)


# ---------------------------------------------------------------------------
# the header and its binding
# ---------------------------------------------------------------------------
def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_xent.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(ENTRIES) | set(QUERIES)
    assert set(ENTRIES) == set(_hip_xent._SIGNATURES) and set(_hip_xent._WS_SIZES) == {QUERIES[0]}
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    from torchkge_amd.csrc import build as hb
    assert 'lp_xent.hip' in hb.SOURCES and hb.EXTRA_FLAGS['lp_xent.hip'] == hb._NO_SLP
    assert any(h.endswith('kge_hip_xent.h') for h in hb.HEADERS)
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    # the sums' contract: no atomic in the source
    code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, 'lp_xent.hip')).read())
    assert not re.search(r'atomic', code, flags=re.I)
    hdr = open(HEADER).read()
    for name, value in (('KGE_XENT_BM', _hip_xent.BM), ('KGE_XENT_BN', _hip_xent.BN),
                        ('KGE_XENT_MIN_TILES_PER_CHUNK', _hip_xent.MIN_TILES_PER_CHUNK),
                        ('KGE_XENT_MAX_CHUNKS', _hip_xent.MAX_CHUNKS), ('KGE_XENT_MAX_K', _hip_xent.MAX_K),
                        ('KGE_XENT_KSLICE', _hip_xent.KSLICE)):
        m = re.search(r'#define %s (\d+)' % name, hdr)
        assert m and int(m.group(1)) == value, name


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
    assert set(protos) == set(ENTRIES) | {'kge_lp_xent_chunks'}
    lib = _hip_xent.load_library()
    for name, args in _hip_xent._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            assert a is kind(prm), (name, prm)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    f = lib.kge_lp_xent_ws_bytes
    assert f.argtypes == [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int] and f.restype is ctypes.c_size_t
    assert re.search(r'\bsize_t\s+kge_lp_xent_ws_bytes\s*\(\s*int64_t \w+,\s*int64_t \w+,\s*int \w+,\s*int \w+\s*\)\s*;',
                     open(HEADER).read())
    assert [kind(p) for p in protos['kge_lp_xent_chunks'].split(',')] == [ctypes.c_int64]
    assert lib.kge_lp_xent_chunks.argtypes == [ctypes.c_int64] and lib.kge_lp_xent_chunks.restype is ctypes.c_int


def test_the_main_header_does_not_know_the_entries():
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    for name in ENTRIES + QUERIES:
        assert name.encode() not in raw
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


# ---------------------------------------------------------------------------
# geometry and workspace (host arithmetic: a process without a GPU)
# ---------------------------------------------------------------------------
def test_chunks_is_a_capped_function_of_n():
    BN, MT, CAP = _hip_xent.BN, _hip_xent.MIN_TILES_PER_CHUNK, _hip_xent.MAX_CHUNKS
    assert [_hip_xent.chunks(n) for n in (-3, 0)] == [0, 0]
    assert [_hip_xent.chunks(n) for n in (1, 2, BN, BN + 1, MT * BN)] == [1] * 5
    assert _hip_xent.chunks(MT * BN + 1) == 2 and _hip_xent.chunks(2 * MT * BN) == 2 and _hip_xent.chunks(2 * MT * BN + 1) == 3
    prev = 0
    for n in [1, 63, 64, 65, 257, 1000, 14951, 40943, 10 ** 6, 1 << 20, 1 << 24, (1 << 31) - 1]:
        c = _hip_xent.chunks(n)
        assert 1 <= c <= CAP and c >= prev and c == min(CAP, -(-(-(-n // BN)) // MT)), n
        prev = c
    assert _hip_xent.chunks(MT * BN * (CAP - 1) + 1) == CAP == _hip_xent.chunks(1 << 30)


def test_workspace_is_bounded_over_n():
    f = _hip_xent.load_library().kge_lp_xent_ws_bytes
    # refusals: 0
    for B, N, K0, K1 in ((0, 10, 4, 0), (-1, 10, 4, 0), (5, 0, 4, 0), (5, -2, 4, 0), (5, 10, 0, 0), (5, 10, 4, -1),
                         (5, 10, 1025, 0), (5, 10, 513, 512), (1 << 31, 10, 4, 0), (5, 1 << 31, 4, 0)):
        assert int(f(B, N, K0, K1)) == 0, (B, N, K0, K1)
    assert int(f(5, 10, 1024, 0)) > 0 and int(f(5, 10, 512, 512)) > 0
    # monotone in B, the documented formula
    for N, K0, K1 in ((1, 1, 0), (300, 20, 0), (14951, 200, 0), (1 << 20, 512, 512)):
        prev = 0
        c = _hip_xent.chunks(N)
        for B in (1, 2, 63, 64, 65, 133, 2048):
            b = int(f(B, N, K0, K1))
            assert b > prev and b % 4 == 0, (B, N)
            assert b == 16 * B * c + (4 * B + 15) // 16 * 16 + 4 * c * B * (K0 + K1)
            prev = b
    # bounded over N: the same bytes at 2^20 and 2^24 candidates, far below one (B, N) fp32 matrix
    for B, K0, K1 in ((1, 8, 0), (2048, 200, 0), (2048, 512, 512)):
        a, b = int(f(B, 1 << 20, K0, K1)), int(f(B, 1 << 24, K0, K1))
        assert a == b > 0
        assert a < 4 * B * (1 << 20)
        assert a == int(f(B, (1 << 31) - 1, K0, K1))
    assert _hip_xent.ws_bytes(70, 300, 20) == int(f(70, 300, 20, 0)) and (70, 300, 20, 0) in _hip_xent._WS_BYTES


# ---------------------------------------------------------------------------
# what the Python layer refuses
# ---------------------------------------------------------------------------
def test_host_tensors_are_refused_before_any_launch():
    Q, E, t = torch.zeros(3, 4), torch.zeros(5, 4), torch.zeros(3, dtype=torch.long)
    with pytest.raises(RuntimeError, match='MI355X'):
        one_vs_all.all_candidates_cross_entropy(Q, E, t)
    with pytest.raises(RuntimeError, match='MI355X'):
        one_vs_all.all_candidates_cross_entropy((Q, Q), (E, E), t, label_smoothing=0.1, reduction='sum')
    for model in (tk.DistMultModel(4, 11, 3), tk.ComplExModel(4, 11, 3)):
        with pytest.raises(RuntimeError, match='MI355X'):
            model.one_vs_all_loss(t, t, t)


def test_bad_arguments_raise_value_errors():
    Q, E, t = torch.zeros(3, 4), torch.zeros(5, 4), torch.zeros(3, dtype=torch.long)
    with pytest.raises(ValueError, match='reduction'):
        one_vs_all.all_candidates_cross_entropy(Q, E, t, reduction='batchmean')
    for eps in (-0.1, 1.5):
        with pytest.raises(ValueError, match='label_smoothing'):
            one_vs_all.all_candidates_cross_entropy(Q, E, t, label_smoothing=eps)
    with pytest.raises(ValueError, match='one matrix or a pair'):
        one_vs_all.all_candidates_cross_entropy((Q, Q, Q), (E, E, E), t)
    for model in (tk.DistMultModel(4, 11, 3), tk.ComplExModel(4, 11, 3)):
        for side in ('tails', 'relation', None):
            with pytest.raises(ValueError, match="'both', 'tail' or 'head'"):
                model.one_vs_all_loss(t, t, t, side=side)
    kg = small_kg()
    model = tk.DistMultModel(4, 11, 3)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    with pytest.raises(ValueError, match="'both', 'tail' or 'head'"):
        OneVsAllTrainer(model, kg, 2, 5, opt, side='left')
    for use_cuda in (None, 'cpu'):
        with pytest.raises(ValueError, match='live on the GPU'):
            OneVsAllTrainer(model, kg, 2, 5, opt, use_cuda=use_cuda)


def test_models_without_the_criterion_name_the_two_that_have_it():
    t = torch.zeros(3, dtype=torch.long)
    kg = small_kg()
    others = [tk.TransEModel(4, 11, 3, 'L2'), tk.TransHModel(4, 11, 3), tk.RESCALModel(4, 11, 3), tk.HolEModel(4, 11, 3),
              tk.AnalogyModel(4, 11, 3)]
    for model in others:
        with pytest.raises(NotImplementedError, match='DistMultModel and ComplExModel') as e:
            model.one_vs_all_loss(t, t, t)
        assert type(model).__name__ in str(e.value)
        with pytest.raises(NotImplementedError, match='DistMultModel and ComplExModel'):
            OneVsAllTrainer(model, kg, 2, 5, torch.optim.SGD(model.parameters(), lr=0.1))


def test_row_optimizers_are_refused_and_the_trainer_keeps_its_arguments():
    kg = small_kg()
    model = tk.ComplExModel(4, 11, 3)
    for cls in (optim.RowSGD, optim.RowAdagrad, optim.RowAdam):
        with pytest.raises(ValueError, match='dense') as e:
            OneVsAllTrainer(model, kg, 2, 5, cls(model.parameters(), lr=0.1))
        assert cls.__name__ in str(e.value) and 'torch.optim' in str(e.value)
    opt = torch.optim.Adagrad(model.parameters(), lr=0.1)
    tr = OneVsAllTrainer(model, kg, 2, 5, opt, 0.1, 'tail', verbose=False)
    assert (tr.n_epochs, tr.batch_size, tr.label_smoothing, tr.side, tr.use_cuda, tr.n_triples) == (2, 5, 0.1, 'tail', 'all', 23)
    assert tr.epoch_losses == [] and tr.sync_free is False and tr.optimizer is opt
    d = OneVsAllTrainer(model, kg, 2, 5, opt)
    assert (d.label_smoothing, d.side, d.use_cuda) == (0.0, 'both', 'all')
    # Trainer itself is as it was: it still takes a criterion and a sampling type
    import inspect
    assert list(inspect.signature(Trainer.__init__).parameters)[:8] == ['self', 'model', 'criterion', 'kg_train', 'n_epochs',
                                                                       'batch_size', 'optimizer', 'sampling_type']
