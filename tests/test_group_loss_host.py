"""CPU-only tests of training with K negatives per fact: the exports, constants and ctypes signatures of
include/kge_hip_group.h, its chunk count and workspace bound, the float64 yardstick (tests/group_loss_ref.py) against
torch's stock operators, the loader's slicing with ``n_neg > 1`` on host tensors, the unchanged leading parameters of
corrupt_kg / TrainDataLoader / Trainer, and what the criteria and the Trainer refuse."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import ROOT
from tests.group_loss_ref import KINDS, forms64, stock, written_out

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_group, sampling
from torchkge_amd.utils import group_losses, losses
from torchkge_amd.utils.training import Trainer, TrainDataLoader

HEADER = os.path.join(ROOT, 'include', 'kge_hip_group.h')
ENTRIES = ('kge_group_loss',)
QUERIES = ('kge_group_loss_ws_bytes', 'kge_group_loss_chunks')
R, S, C, M = _hip_group.ROWS, _hip_group.SLICES, _hip_group.MIN_K_PER_CHUNK, _hip_group.MAX_CHUNKS


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def prototypes():
    return dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', header_text(), flags=re.S))


# ---------------------------------------------------------------------------
# the header and its binding
# ---------------------------------------------------------------------------
def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_group.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(ENTRIES) | set(QUERIES)
    assert set(ENTRIES) == set(_hip_group._SIGNATURES) and set(_hip_group._WS_SIZES) == {QUERIES[0]}
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    for name in declared:
        assert hasattr(lib, name), name
    from torchkge_amd.csrc import build as hb
    assert 'group_loss.hip' in hb.SOURCES and '-ffp-contract=off' in hb.FLAGS and 'group_loss.hip' not in hb.EXTRA_FLAGS
    assert any(h.endswith('kge_hip_group.h') for h in hb.HEADERS) and 'loss_common.h' in hb.HEADERS
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    # the contract: no atomic in the source or in what it shares with pair_loss.hip, and one summation tree behind both
    for name in ('group_loss.hip', 'loss_common.h'):
        code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, name)).read())
        assert not re.search(r'atomic', code, flags=re.I), name
    for name in ('group_loss.hip', 'pair_loss.hip'):
        code = open(os.path.join(hb.HERE, name)).read()
        assert '#include "loss_common.h"' in code and 'st_thread_sum(' in code and '__shfl_xor' not in code, name
    hdr = open(HEADER).read()
    for name, value in (('KGE_GROUP_NSSA', _hip_group.GROUP_NSSA), ('KGE_GROUP_SOFTMAX', _hip_group.GROUP_SOFTMAX),
                        ('KGE_GROUP_ROWS', R), ('KGE_GROUP_SLICES', S), ('KGE_GROUP_MIN_K_PER_CHUNK', C),
                        ('KGE_GROUP_MAX_CHUNKS', M)):
        m = re.search(r'#define %s (\d+)' % name, hdr)
        assert m and int(m.group(1)) == value, name
    assert (_hip_group.GROUP_NSSA, _hip_group.GROUP_SOFTMAX) == (0, 1)
    assert R % 64 == 0 and S >= 2 and C >= 2 and M >= 2


def test_ctypes_signatures_match_the_header_prototypes():
    protos = prototypes()

    def kind(param):
        param = param.strip()
        if '*' in param:
            return ctypes.c_void_p
        t = param.split()
        if 'kge_stream_t' in t:
            return ctypes.c_void_p
        if 'int64_t' in t:
            return ctypes.c_int64
        if 'size_t' in t:
            return ctypes.c_size_t
        if 'float' in t:
            return ctypes.c_float
        if 'int' in t:
            return ctypes.c_int
        raise AssertionError('unparsed parameter: %r' % param)
    assert set(protos) == {'kge_group_loss', 'kge_group_loss_chunks'}
    for name, args in _hip_group._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            assert a is kind(prm), (name, prm)
    lib = _hip_group.load_library()
    for name, args in _hip_group._SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    f = lib.kge_group_loss_ws_bytes
    assert f.argtypes == [ctypes.c_int64, ctypes.c_int64] and f.restype is ctypes.c_size_t
    assert re.search(r'\bsize_t\s+kge_group_loss_ws_bytes\s*\(\s*int64_t \w+\s*,\s*int64_t \w+\s*\)\s*;', open(HEADER).read())
    assert [kind(p) for p in protos['kge_group_loss_chunks'].split(',')] == [ctypes.c_int64]
    assert lib.kge_group_loss_chunks.argtypes == [ctypes.c_int64] and lib.kge_group_loss_chunks.restype is ctypes.c_int


def test_the_main_header_does_not_know_the_entry():
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    for name in ENTRIES + QUERIES:
        assert name.encode() not in raw
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


def test_chunk_count_and_workspace_bound():
    chunks, ws = _hip_group.chunks, _hip_group.load_library().kge_group_loss_ws_bytes     # (host arithmetic: no GPU)
    assert [chunks(k) for k in (-3, 0)] == [0, 0]
    assert all(chunks(k) == 1 for k in range(1, C + 1)) and chunks(C + 1) == 2
    prev = 0
    for k in list(range(1, 4 * C)) + [M * C - 1, M * C, M * C + 1, 2 * M * C + 3, 1 << 20, (1 << 31) - 1]:
        c = chunks(k)
        assert prev <= c <= M and c == min(-(-k // C), M) and c <= k, k
        prev = c
    assert chunks(M * C) == M == chunks(1 << 30)
    # the header's split: chunks are never empty, and slices only where one chunk holds fewer negatives than slices
    for k in list(range(1, 6 * C)) + [M * C - 1, M * C + 1, 2 * M * C + 3]:
        c = chunks(k)
        bounds = [i * k // c for i in range(c + 1)]
        assert bounds[0] == 0 and bounds[-1] == k and all(b > a for a, b in zip(bounds, bounds[1:])), k
        for k0, k1 in zip(bounds, bounds[1:]):
            cuts = [k0 + s * (k1 - k0) // S for s in range(S + 1)]
            assert cuts[0] == k0 and cuts[-1] == k1
            assert all(b > a for a, b in zip(cuts, cuts[1:])) or (c == 1 and k < S), k
    # bad arguments
    for B, K in ((0, 5), (-1, 5), (5, 0), (5, -1), (1 << 16, 1 << 15), (1, 1 << 31), (1 << 31, 1), (1 << 40, 1 << 40)):
        assert int(ws(B, K)) == 0, (B, K)
    assert int(ws((1 << 31) - 1, 1)) > 0 and int(ws(1, (1 << 31) - 1)) > 0
    # monotone in B (and in K), 16-byte granular, and no B * K-sized term: a constant per fact whatever K
    per_fact = 20 * S * M + 8
    for K in (1, 2, C, C + 1, M * C, 1 << 20):
        prev = 0
        for B in list(range(1, 40)) + [R - 1, R, R + 1, 1023, 1024, 1025, 4096, 1 << 20]:
            if B * K >= 1 << 31:
                continue
            b = int(ws(B, K))
            assert b >= prev and b % 16 == 0 and b >= 16, (B, K)
            assert b <= per_fact * (B + R - 1) + 8 * 1024 + 16, (B, K)
            assert b >= int(ws(B, max(K // 2, 1))), (B, K)
            prev = b
    assert int(ws(1000, 1 << 20)) == int(ws(1000, M * C))
    assert _hip_group.ws_bytes(77, 5) == int(ws(77, 5)) and (77, 5) in _hip_group._WS_BYTES


# ---------------------------------------------------------------------------
# the yardstick is torch's stock operators
# ---------------------------------------------------------------------------
def scores64(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    pos = (torch.rand(B, generator=g, dtype=torch.float64) * 20 - 10).float()
    neg = (torch.rand(K, B, generator=g, dtype=torch.float64) * 20 - 10).float()
    pos[:2], neg[0, :2], neg[1, :2] = torch.tensor([10.0, -10.0]), torch.tensor([-10.0, 10.0]), torch.tensor([10.0, 10.0])
    return pos, neg


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('kind', KINDS)
def test_the_float64_forms_are_the_stock_operators(kind, weighted):
    B, K, margin = 301, 37, 1.5
    pos, neg = scores64(B, K, 5)
    w = (torch.rand(B, generator=torch.Generator().manual_seed(6)) + 0.25).double() if weighted else None
    for alpha in (0.0, 0.5, 1.0):
        row64, l64, dp64, dn64 = forms64(kind, margin, alpha, pos, neg, w)
        row, loss, dp, dn = stock(kind, margin, alpha, pos.double(), neg.double(), w)
        assert abs(float(loss) - float(l64)) <= 1e-12 * abs(float(l64)), (kind, alpha)
        assert float((row - row64).abs().max()) <= 1e-12 * float(row64.abs().max())
        assert float((dp - dp64).abs().max()) <= 1e-12 and float((dn - dn64).abs().max()) <= 1e-12, (kind, alpha)
    # the written-out softmax criterion IS cross_entropy on cat([pos, neg]) with target 0, the NSSA one logsigmoid under
    # detached softmax weights
    p, x = pos.double(), neg.double()
    ce = F.cross_entropy(torch.cat([p.view(-1, 1), x.t()], 1), torch.zeros(B, dtype=torch.long), reduction='sum')
    assert abs(float(ce) - float(forms64('softmax', 0.0, 0.0, pos, neg)[1])) <= 1e-12 * float(ce)
    wts = F.softmax(0.5 * x, 0).detach()
    ns = (-F.logsigmoid(margin + p) - (wts * F.logsigmoid(-margin - x)).sum(0)).sum()
    assert abs(float(ns) - float(forms64('nssa', margin, 0.5, pos, neg)[1])) <= 1e-12 * float(ns)
    assert torch.equal(written_out('nssa', margin, 0.5, p, x).sum(), ns)


def test_temperature_zero_is_the_plain_mean_over_the_negatives():
    pos, neg = scores64(65, 9, 7)
    margin = 2.0
    row, loss, dp, dn = forms64('nssa', margin, 0.0, pos, neg)
    p, x = pos.double(), neg.double()
    want = F.softplus(-(margin + p)) + F.softplus(margin + x).mean(dim=0)
    assert float((row - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((dn - torch.sigmoid(margin + x) / 9).abs().max()) <= 1e-12
    assert float((dp + torch.sigmoid(-(margin + p))).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------
# the loader with n_neg > 1, on the host
# ---------------------------------------------------------------------------
class Replay(object):
    """A sampler that hands out recorded negatives; its corrupt_kg has the NEW signature and records n_neg."""

    def __init__(self, epochs):
        self.epochs, self.calls, self.sync_free = list(epochs), [], False

    def corrupt_kg(self, batch_size, use_cuda, which='main', on_device=False, *, n_neg=1):
        nh, nt = self.epochs[len(self.calls) % len(self.epochs)]
        self.calls.append((batch_size, use_cuda, on_device, n_neg))
        return nh.clone(), nt.clone()


class OldReplay(object):
    """The replay sampler of the older suites: no ``n_neg`` in its signature."""

    def __init__(self, nh, nt):
        self.nh, self.nt, self.calls, self.sync_free = nh, nt, 0, False

    def corrupt_kg(self, batch_size, use_cuda, which='main', on_device=False):
        self.calls += 1
        return self.nh.clone(), self.nt.clone()


def small_kg(n=23, n_ent=11, n_rel=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    h, t, r = (torch.randint(0, m, (n,), generator=g) for m in (n_ent, n_ent, n_rel))
    return tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                             rel2ix={i: i for i in range(n_rel)})


def test_loader_hands_every_batch_its_own_block_of_negatives():
    kg = small_kg()
    n, b, k = 23, 5, 3
    sizes = [5, 5, 5, 5, 3]
    g = torch.Generator().manual_seed(1)
    # recorded per batch, so that the expected block of a batch is known by construction
    blocks = [[(torch.randint(0, 11, (k * s,), generator=g), torch.randint(0, 11, (k * s,), generator=g)) for s in sizes]
              for _ in range(2)]
    epochs = [(torch.cat([x[0] for x in ep]), torch.cat([x[1] for x in ep])) for ep in blocks]
    assert epochs[0][0].shape[0] == k * n
    sampler = Replay(epochs)
    loader = TrainDataLoader(kg, b, 'ignored', use_cuda=None, sampler=sampler, n_neg=k)
    assert loader.n_neg == k and len(loader) == 5 and loader.get_counter_examples() is None
    for e in range(2):
        batches = list(loader)
        assert sampler.calls == [(b, False, False, k)] * (e + 1)
        assert [x['h'].shape[0] for x in batches] == sizes
        for i, batch in enumerate(batches):
            sl = slice(b * i, b * i + b)
            assert torch.equal(batch['h'], kg.head_idx[sl]) and torch.equal(batch['r'], kg.relations[sl])
            assert torch.equal(batch['nh'], blocks[e][i][0]) and torch.equal(batch['nt'], blocks[e][i][1]), (e, i)
            assert batch['nh'].shape[0] == k * sizes[i]
        ce = loader.get_counter_examples()
        assert isinstance(ce, tk.SmallKG) and len(ce) == k * n
        assert ce.head_idx.shape == ce.tail_idx.shape == ce.relations.shape == (k * n,)
        assert torch.equal(ce.head_idx, epochs[e][0]) and torch.equal(ce.tail_idx, epochs[e][1])
        want_r = torch.cat([kg.relations[b * i:b * i + b].repeat(k) for i in range(5)])
        assert torch.equal(ce.relations, want_r)
    with pytest.raises(ValueError, match='n_neg'):
        TrainDataLoader(kg, b, 'bern', sampler=sampler, n_neg=0)


def test_an_old_signature_sampler_still_serves_one_negative_per_fact():
    kg = small_kg()
    g = torch.Generator().manual_seed(2)
    nh, nt = torch.randint(0, 11, (23,), generator=g), torch.randint(0, 11, (23,), generator=g)
    old = OldReplay(nh, nt)
    for loader in (TrainDataLoader(kg, 5, 'x', sampler=old), TrainDataLoader(kg, 5, 'x', sampler=old, n_neg=1)):
        batches = list(loader)
        assert torch.equal(torch.cat([b['nh'] for b in batches]), nh) and torch.equal(torch.cat([b['nt'] for b in batches]), nt)
        ce = loader.get_counter_examples()
        assert len(ce) == 23 and torch.equal(ce.relations, kg.relations)
    assert old.calls == 2
    with pytest.raises(TypeError, match='n_neg'):
        list(TrainDataLoader(kg, 5, 'x', sampler=old, n_neg=2))


def test_leading_parameters_are_unchanged_and_the_new_keyword_defaults_to_one():
    for cls in (sampling.NegativeSampler, sampling.UniformNegativeSampler, sampling.BernoulliNegativeSampler,
                sampling.PositionalNegativeSampler, sampling.BernoulliRelationNegativeSampler):
        p = inspect.signature(cls.corrupt_kg).parameters
        assert list(p) == ['self', 'batch_size', 'use_cuda', 'which', 'on_device', 'n_neg'], cls.__name__
        assert p['n_neg'].default == 1 and p['n_neg'].kind is inspect.Parameter.KEYWORD_ONLY
        assert p['on_device'].default is False and p['which'].default == 'main'
    p = inspect.signature(TrainDataLoader.__init__).parameters
    assert list(p) == ['self', 'kg', 'batch_size', 'sampling_type', 'use_cuda', 'sampler', 'sync_free', 'n_neg']
    assert p['n_neg'].default == 1 and p['n_neg'].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(Trainer.__init__).parameters
    assert list(p) == ['self', 'model', 'criterion', 'kg_train', 'n_epochs', 'batch_size', 'optimizer', 'sampling_type',
                       'use_cuda', 'fused', 'sync_free', 'sampler', 'verbose', 'n_neg']
    assert p['n_neg'].default == 1 and p['n_neg'].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(_hip_group.group_loss).parameters
    assert list(p) == ['kind', 'margin', 'temperature', 'pos', 'neg', 'n_neg', 'weights', 'acc', 'need_grad']
    p = inspect.signature(group_losses.SelfAdversarialLoss.__init__).parameters
    assert list(p) == ['self', 'margin', 'temperature', 'n_neg', 'reduction']
    assert (p['temperature'].default, p['n_neg'].default, p['reduction'].default) == (1.0, None, 'sum')
    p = inspect.signature(group_losses.SampledSoftmaxLoss.__init__).parameters
    assert list(p) == ['self', 'n_neg', 'reduction'] and (p['n_neg'].default, p['reduction'].default) == (None, 'sum')
    p = inspect.signature(group_losses.SelfAdversarialLoss.forward).parameters
    assert list(p) == ['self', 'positive_triplets', 'negative_triplets', 'acc', 'weights']


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_the_criteria_refuse_host_tensors_bad_lengths_and_an_unset_n_neg():
    for crit in (group_losses.SelfAdversarialLoss(6.0, 1.0, n_neg=3), group_losses.SampledSoftmaxLoss(n_neg=3)):
        assert isinstance(crit, torch.nn.Module) and crit.n_neg == 3 and crit.reduction == 'sum'
        with pytest.raises(RuntimeError, match='MI355X'):       # before any launch: there is no GPU here
            crit(torch.zeros(4), torch.zeros(12))
        with pytest.raises(RuntimeError, match='MI355X'):
            crit(torch.zeros(12), torch.zeros(12))              # the repeated form
        with pytest.raises(ValueError, match='not 3 per fact'):
            crit(torch.zeros(4), torch.zeros(13))
        with pytest.raises(ValueError, match='positive scores'):
            crit(torch.zeros(5), torch.zeros(12))
    for crit in (group_losses.SelfAdversarialLoss(6.0), group_losses.SampledSoftmaxLoss()):
        assert crit.n_neg is None
        with pytest.raises(ValueError, match='needs n_neg'):
            crit(torch.zeros(4), torch.zeros(12))
    a = group_losses.SelfAdversarialLoss(6, temperature=0.5, n_neg=2, reduction='mean')
    assert (a.margin, a.temperature, a.kind, a.reduction) == (6.0, 0.5, _hip_group.GROUP_NSSA, 'mean')
    assert group_losses.SampledSoftmaxLoss().kind == _hip_group.GROUP_SOFTMAX
    for bad in (-0.5, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='temperature'):
            group_losses.SelfAdversarialLoss(6.0, temperature=bad)
    with pytest.raises(ValueError, match='reduction'):
        group_losses.SampledSoftmaxLoss(reduction='none')
    with pytest.raises(ValueError, match='n_neg'):
        group_losses.SampledSoftmaxLoss(n_neg=0)
    # the pairwise criteria and their mapping are untouched
    from torchkge_amd.utils import fused_losses
    assert fused_losses.fused_for(a) is None and type(fused_losses.fused_for(losses.MarginLoss(1.0))) is fused_losses.FusedMarginLoss


def test_trainer_sets_or_checks_the_criterions_n_neg():
    kg = small_kg()
    model = tk.TransEModel(4, 11, 3, 'L2')
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    crit = group_losses.SelfAdversarialLoss(6.0)
    tr = Trainer(model, crit, kg, 2, 5, opt, use_cuda='all', n_neg=4, verbose=False)
    assert crit.n_neg == 4 and tr.n_neg == 4 and tr._fused_criterion is None and tr._grouped
    Trainer(model, crit, kg, 2, 5, opt, use_cuda='all', n_neg=4)             # the same value again
    with pytest.raises(ValueError, match='4 negatives per fact, the Trainer draws 2'):
        Trainer(model, crit, kg, 2, 5, opt, use_cuda='all', n_neg=2)
    with pytest.raises(ValueError, match='the Trainer draws 1'):
        Trainer(model, group_losses.SampledSoftmaxLoss(n_neg=8), kg, 2, 5, opt, use_cuda='all')
    with pytest.raises(ValueError, match='n_neg'):
        Trainer(model, crit, kg, 2, 5, opt, use_cuda='all', n_neg=0)
    # a pairwise criterion keeps its fused counterpart with more negatives
    tr = Trainer(model, losses.MarginLoss(0.5), kg, 2, 5, opt, use_cuda='all', n_neg=4)
    assert tr.n_neg == 4 and not tr._grouped and tr._fused_criterion is not None
    assert Trainer(model, losses.MarginLoss(0.5), kg, 2, 5, opt, use_cuda='all').n_neg == 1
