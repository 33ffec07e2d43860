"""CPU-only tests of the training loop: the exports and ctypes signatures of include/kge_hip_train.h, its workspace
bound, TrainDataLoader on host tensors with a replaying sampler, fused_for, what Trainer refuses, the names that
torchkge_amd.utils still leaves out, and the records of tests/golden/ref_trainer.npz."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, GOLDEN

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_train
from torchkge_amd.utils import fused_losses, losses
from torchkge_amd.utils.training import Trainer, TrainDataLoader

HEADER = os.path.join(ROOT, 'include', 'kge_hip_train.h')
ENTRIES = ('kge_pair_loss',)
QUERIES = ('kge_pair_loss_ws_bytes', 'kge_pair_loss_max_blocks')


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def prototypes():
    return dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', header_text(), flags=re.S))


class Replay(object):
    """A sampler that hands out recorded negatives, one (nh, nt) pair per corrupt_kg call, and counts the calls."""

    def __init__(self, epochs):
        self.epochs, self.calls, self.sync_free = list(epochs), [], False

    def corrupt_kg(self, batch_size, use_cuda, which='main', on_device=False):
        nh, nt = self.epochs[len(self.calls) % len(self.epochs)]
        self.calls.append((batch_size, use_cuda, on_device))
        return (nh.cuda(), nt.cuda()) if on_device else (nh.clone(), nt.clone())


def small_kg(n=23, n_ent=11, n_rel=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    h, t, r = (torch.randint(0, m, (n,), generator=g) for m in (n_ent, n_ent, n_rel))
    return tk.KnowledgeGraph(kg={'heads': h, 'tails': t, 'relations': r}, ent2ix={i: i for i in range(n_ent)},
                             rel2ix={i: i for i in range(n_rel)})


# ---------------------------------------------------------------------------
# the header and its binding
# ---------------------------------------------------------------------------
def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_train.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(ENTRIES) | set(QUERIES)
    assert set(ENTRIES) == set(_hip_train._SIGNATURES) and set(_hip_train._WS_SIZES) == {QUERIES[0]}
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    for name in declared:
        assert hasattr(lib, name), name
    from torchkge_amd.csrc import build as hb
    assert 'pair_loss.hip' in hb.SOURCES and '-ffp-contract=off' in hb.FLAGS and 'pair_loss.hip' not in hb.EXTRA_FLAGS
    assert any(h.endswith('kge_hip_train.h') for h in hb.HEADERS)
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    # the sum's contract: no atomic in the source
    code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, 'pair_loss.hip')).read())
    assert not re.search(r'atomic', code, flags=re.I)
    hdr = open(HEADER).read()
    for name, value in (('KGE_LOSS_MARGIN', _hip_train.LOSS_MARGIN), ('KGE_LOSS_LOGISTIC', _hip_train.LOSS_LOGISTIC),
                        ('KGE_LOSS_BCE', _hip_train.LOSS_BCE), ('KGE_PAIR_LOSS_CHUNK', _hip_train.CHUNK)):
        m = re.search(r'#define %s (\d+)' % name, hdr)
        assert m and int(m.group(1)) == value, name
    assert (_hip_train.LOSS_MARGIN, _hip_train.LOSS_LOGISTIC, _hip_train.LOSS_BCE) == (0, 1, 2)
    assert _hip_train.CHUNK % 256 == 0


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
    assert set(protos) == {'kge_pair_loss', 'kge_pair_loss_max_blocks'}
    for name, args in _hip_train._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            assert a is kind(prm), (name, prm)
    lib = _hip_train.load_library()
    for name, args in _hip_train._SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    f = lib.kge_pair_loss_ws_bytes
    assert f.argtypes == [ctypes.c_int64] and f.restype is ctypes.c_size_t
    assert re.search(r'\bsize_t\s+kge_pair_loss_ws_bytes\s*\(\s*int64_t \w+\s*\)\s*;', open(HEADER).read())
    assert protos['kge_pair_loss_max_blocks'].strip() == 'void'
    assert lib.kge_pair_loss_max_blocks.argtypes == [] and lib.kge_pair_loss_max_blocks.restype is ctypes.c_int


def test_the_main_header_does_not_know_the_entry():
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    for name in ENTRIES + QUERIES:
        assert name.encode() not in raw
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


def test_workspace_bound_and_grid_cap():
    f = _hip_train.load_library().kge_pair_loss_ws_bytes         # (a process without a GPU: host arithmetic)
    assert [int(f(n)) for n in (-5, -1, 0, 1 << 31, 1 << 40)] == [0, 0, 0, 0, 0]
    cap, chunk = _hip_train.max_blocks(), _hip_train.CHUNK
    assert cap >= 1
    prev = 0
    for n in list(range(1, 70)) + [chunk - 1, chunk, chunk + 1, 32768 + 105, cap * chunk - 1, cap * chunk, cap * chunk + 1,
                                   (1 << 31) - 1]:
        b = int(f(n))
        assert b >= 8 and b >= prev and b % 8 == 0, n
        assert b == 8 * min(-(-n // chunk), cap), n         # one fp64 partial per block of the first stage
        prev = b
    assert _hip_train.ws_bytes(2053) == int(f(2053)) and 2053 in _hip_train._WS_BYTES


# ---------------------------------------------------------------------------
# TrainDataLoader on the host
# ---------------------------------------------------------------------------
def test_loader_batches_slices_and_fresh_negatives_per_iteration():
    kg = small_kg()
    g = torch.Generator().manual_seed(1)
    epochs = [(torch.randint(0, 11, (23,), generator=g), torch.randint(0, 11, (23,), generator=g)) for _ in range(2)]
    sampler = Replay(epochs)
    loader = TrainDataLoader(kg, 5, 'no such type', use_cuda=None, sampler=sampler)     # sampling_type is ignored
    assert loader.sampler is sampler and len(loader) == 5 and not sampler.calls
    assert loader.get_counter_examples() is None
    for e in range(3):
        batches = list(loader)
        assert sampler.calls == [(5, False, False)] * (e + 1)           # one corruption of the whole graph per __iter__
        nh, nt = epochs[e % 2]
        assert [b['h'].shape[0] for b in batches] == [5, 5, 5, 5, 3]
        for i, b in enumerate(batches):
            assert sorted(b) == ['h', 'nh', 'nt', 'r', 't']
            sl = slice(5 * i, 5 * i + 5)
            for key, src in (('h', kg.head_idx), ('t', kg.tail_idx), ('r', kg.relations), ('nh', nh), ('nt', nt)):
                assert torch.equal(b[key], src[sl]) and not b[key].is_cuda, (e, i, key)
        ce = loader.get_counter_examples()
        assert isinstance(ce, tk.SmallKG) and len(ce) == 23
        assert torch.equal(ce.head_idx, nh) and torch.equal(ce.tail_idx, nt) and torch.equal(ce.relations, kg.relations)
    assert len(TrainDataLoader(kg, 23, 'bern', sampler=sampler)) == 1 and len(TrainDataLoader(kg, 24, 'bern', sampler=sampler)) == 1
    assert len(TrainDataLoader(kg, 1, 'bern', sampler=sampler)) == 23


def test_loader_builds_the_two_samplers_and_sets_sync_free():
    kg = small_kg()
    assert type(TrainDataLoader(kg, 5, 'unif').sampler) is tk.UniformNegativeSampler
    bern = TrainDataLoader(kg, 5, 'bern')
    assert type(bern.sampler) is tk.BernoulliNegativeSampler and bern.sampler.sync_free is False
    assert TrainDataLoader(kg, 5, 'bern', sync_free=True).sampler.sync_free is True
    s = Replay([(kg.head_idx, kg.tail_idx)])
    TrainDataLoader(kg, 5, 'bern', sampler=s, sync_free=True)
    assert s.sync_free is True
    with pytest.raises(ValueError, match='sampling_type'):
        TrainDataLoader(kg, 5, 'positional')


def test_corrupt_kg_takes_on_device_on_every_sampler():
    import inspect
    from torchkge_amd import sampling
    for cls in (sampling.NegativeSampler, sampling.UniformNegativeSampler, sampling.BernoulliNegativeSampler,
                sampling.PositionalNegativeSampler, sampling.BernoulliRelationNegativeSampler):
        p = inspect.signature(cls.corrupt_kg).parameters
        assert list(p)[:5] == ['self', 'batch_size', 'use_cuda', 'which', 'on_device'], cls.__name__
        assert p['on_device'].default is False and p['which'].default == 'main'


# ---------------------------------------------------------------------------
# the criteria and the Trainer's refusals
# ---------------------------------------------------------------------------
def test_fused_for_maps_the_three_classes_and_nothing_else():
    m = fused_losses.fused_for(losses.MarginLoss(0.25))
    assert type(m) is fused_losses.FusedMarginLoss and m.margin == 0.25 and m.kind == _hip_train.LOSS_MARGIN
    assert type(fused_losses.fused_for(losses.LogisticLoss())) is fused_losses.FusedLogisticLoss
    assert type(fused_losses.fused_for(losses.BinaryCrossEntropyLoss())) is fused_losses.FusedBinaryCrossEntropyLoss
    assert fused_losses.FusedLogisticLoss().kind == _hip_train.LOSS_LOGISTIC
    assert fused_losses.FusedBinaryCrossEntropyLoss().kind == _hip_train.LOSS_BCE
    assert fused_losses.fused_for(lambda p, n: (n - p).sum()) is None
    assert fused_losses.fused_for(torch.nn.MSELoss()) is None
    assert fused_losses.fused_for(m) is None

    class Mine(losses.MarginLoss):          # a subclass may have changed the terms
        pass
    assert fused_losses.fused_for(Mine(0.5)) is None
    for cls in (fused_losses.FusedMarginLoss, fused_losses.FusedLogisticLoss, fused_losses.FusedBinaryCrossEntropyLoss):
        assert issubclass(cls, torch.nn.Module)
    # host tensors are refused before any launch
    with pytest.raises(RuntimeError, match='MI355X'):
        m(torch.zeros(3), torch.zeros(3))


def test_trainer_refuses_a_host_run_and_keeps_its_arguments():
    kg = small_kg()
    model = tk.TransEModel(4, 11, 3, 'L2')
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    for use_cuda in (None, 'cpu'):
        with pytest.raises(ValueError, match='live on the GPU'):
            Trainer(model, losses.MarginLoss(0.5), kg, 2, 5, opt, use_cuda=use_cuda)
    with pytest.raises(ValueError, match='live on the GPU'):
        Trainer(model, losses.MarginLoss(0.5), kg, 2, 5, opt)
    tr = Trainer(model, losses.MarginLoss(0.5), kg, 2, 5, opt, 'unif', 'all', verbose=False)
    assert (tr.n_epochs, tr.batch_size, tr.sampling_type, tr.use_cuda, tr.n_triples) == (2, 5, 'unif', 'all', 23)
    assert tr.get_counter_examples() is None and tr.epoch_losses == [] and tr.fused is True and tr.sync_free is False
    assert type(tr._fused_criterion) is fused_losses.FusedMarginLoss and tr._row_mode is False
    assert Trainer(model, losses.MarginLoss(0.5), kg, 2, 5, opt, use_cuda='all', fused=False)._fused_criterion is None
    assert Trainer(model, torch.nn.MSELoss(), kg, 2, 5, opt, use_cuda='batch')._fused_criterion is None
    from torchkge_amd import optim
    for cls in (optim.RowSGD, optim.RowAdagrad, optim.RowAdam):
        assert Trainer(model, losses.MarginLoss(0.5), kg, 2, 5, cls(model.parameters(), lr=0.1), use_cuda='all')._row_mode


def test_the_utils_names_still_raise_and_point_at_the_module():
    from torchkge_amd import utils
    for name in ('Trainer', 'TrainDataLoader'):
        assert not hasattr(utils, name)
        with pytest.raises(AttributeError, match='does not provide') as e:
            getattr(utils, name)
        assert 'torchkge_amd.utils.training' in str(e.value) and name in str(e.value)
    from torchkge_amd.utils import training
    assert training.Trainer is Trainer and training.TrainDataLoader is TrainDataLoader


# ---------------------------------------------------------------------------
# the fixture's own records
# ---------------------------------------------------------------------------
def test_fixture_records():
    z = np.load(os.path.join(GOLDEN, 'ref_trainer.npz'))
    n = int(z['heads'].shape[0])
    assert (n, int(z['n_ent']), int(z['n_rel']), int(z['b_size']), int(z['n_epochs'])) == (1385, 300, 7, 128, 3)
    assert n % int(z['b_size']) == 105 and float(z['lr']) == 0.01 and float(z['margin']) == 0.5
    for case, n_tables in (('transe', 2), ('distmult', 2), ('complex', 4)):
        # the fp32 and the fp64 run of the reference drew the same negatives
        assert np.array_equal(z[case + '_nh32'], z[case + '_nh64']) and np.array_equal(z[case + '_nt32'], z[case + '_nt64'])
        assert z[case + '_nh32'].shape == (3, n) and z[case + '_loss32'].shape == (3,) == z[case + '_loss64'].shape
        # a fresh corruption per epoch
        assert not np.array_equal(z[case + '_nh32'][0], z[case + '_nh32'][1])
        for i in range(n_tables):
            a, f32, f64 = (z['%s_%s%d' % (case, k, i)] for k in ('init', 'final32_', 'final64_'))
            assert a.dtype == np.float32 == f32.dtype and f64.dtype == np.float64 and a.shape == f32.shape == f64.shape
            assert np.abs(f32 - f64).max() < 1e-5 and np.abs(a - f32).max() > 1e-4      # it trained, both runs alike
        assert '%s_init%d' % (case, n_tables) not in z.files
    # no hinge of the margin case can flip inside float noise
    assert float(z['transe_min_hinge']) >= 1e-4 == float(z['min_hinge_bound'])
