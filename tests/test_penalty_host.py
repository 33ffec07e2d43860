"""CPU-only tests of the embedding regularizers (include/kge_hip_penalty.h): the exports and ctypes signatures, the
descriptor structure, the sizing helpers (offsets with mixed layouts and widths), every KGE_EINVAL of both entries on
never-dereferenced aligned addresses (every refusal happens before a launch), ``_penalty_groups()`` of every model class,
the float64 yardstick against finite differences, and the trainers' attribute."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from tests import penalty_ref as ref
from tests.helpers import ROOT

from torchkge_amd import _hip, _hip_penalty as hp
from torchkge_amd.utils.regularizers import LpRegularizer, N3Regularizer
from torchkge_amd.utils.training import Trainer, OneVsAllTrainer, KvsAllTrainer

HEADER = os.path.join(ROOT, 'include', 'kge_hip_penalty.h')
ENTRIES = ('kge_row_penalty', 'kge_row_penalty_bwd')
QUERIES = ('kge_row_penalty_terms', 'kge_row_penalty_ws_bytes', 'kge_row_penalty_rows_floats', 'kge_row_penalty_row_offset')
EINVAL = -1
A = [4096 * (i + 1) for i in range(16)]     # 16-byte aligned, never dereferenced


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def streams_of(*specs):
    """A ctypes array of kge_penalty_stream from dicts; the defaults are one valid REAL stream."""
    arr = (hp.PenaltyStream * max(len(specs), 1))()
    for q, s in enumerate(specs):
        f = dict(t0=A[0], t1=None, ld=8, d=8, layout=hp.REAL, ids=A[2], n=4, factor=0.25)
        f.update(s)
        arr[q] = hp.PenaltyStream(**f)
    return arr


def test_library_exports_every_symbol_the_header_declares_and_the_build_lists_the_file():
    lib = hp.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(ENTRIES) | set(QUERIES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    from torchkge_amd.csrc import build as hb
    assert 'row_penalty.hip' in hb.SOURCES and 'row_penalty.hip' not in hb.EXTRA_FLAGS
    assert 'loss_common.h' in hb.HEADERS and any(h.endswith('kge_hip_penalty.h') for h in hb.HEADERS)
    code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, 'row_penalty.hip')).read())
    assert '#include "loss_common.h"' in code and not re.search(r'atomic', code, flags=re.I)      # one tree, no float atomic
    for name, value in (('REAL', hp.REAL), ('SPLIT', hp.SPLIT), ('INTERLEAVED', hp.INTERLEAVED), ('MAX_STREAMS', hp.MAX_STREAMS),
                        ('WAVES', hp.WAVES), ('MAX_BLOCKS', hp.MAX_BLOCKS)):
        m = re.search(r'#define KGE_PENALTY_%s (\d+)' % name, open(HEADER).read())
        assert m and int(m.group(1)) == value, name
    assert (ref.REAL, ref.SPLIT, ref.INTERLEAVED) == (hp.REAL, hp.SPLIT, hp.INTERLEAVED)
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    for name in ENTRIES + QUERIES:
        assert name.encode() not in raw and name not in _hip._SIGNATURES
    assert _hip.ABI_VERSION == 33 and int(lib.kge_abi_version()) == 33


def test_ctypes_signatures_and_the_structure_match_the_header():
    text = header_text()
    protos = {name: (ret, params) for ret, name, params in
              re.findall(r'\b(int|int64_t|size_t)\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', text, flags=re.S)}

    def kind(param):
        t = param.strip().split()
        if '*' in param or 'kge_stream_t' in t:
            return ctypes.c_void_p
        for name, c in (('size_t', ctypes.c_size_t), ('int64_t', ctypes.c_int64), ('int', ctypes.c_int), ('float', ctypes.c_float)):
            if name in t:
                return c
        raise AssertionError('unparsed parameter: %r' % param)
    returns = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t}
    assert set(protos) == set(hp._SIGNATURES) | set(hp._QUERIES)
    lib = hp.load_library()
    for name, args in hp._SIGNATURES.items():
        ret, params = protos[name]
        assert ret == 'int' and [kind(p) for p in params.split(',')] == args, name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    for name, (args, res) in hp._QUERIES.items():
        ret, params = protos[name]
        assert returns[ret] is res and [kind(p) for p in params.split(',')] == args, name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    body = re.search(r'typedef struct kge_penalty_stream \{(.*?)\} kge_penalty_stream;', text, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names = [n.strip() for n in decl.split(',')]
            first = names[0].split()
            ctype = kind(decl)
            fields += [(first[-1].lstrip('*'), ctype)] + [(n.lstrip('*'), ctype) for n in names[1:]]
    assert fields == [(n, c) for n, c in hp.PenaltyStream._fields_]
    assert ctypes.sizeof(hp.PenaltyStream) == 56


def test_sizing_helpers_with_mixed_layouts_and_widths():
    lib = hp.load_library()
    arr = streams_of(dict(d=5, ld=8, n=7), dict(layout=hp.SPLIT, t1=A[1], d=64, ld=64, n=3),
                     dict(layout=hp.INTERLEAVED, d=10, ld=12, n=2), dict(n=0), dict(d=1030, ld=1030, n=300))
    sizes = [7 * 5, 2 * 3 * 64, 2 * 10, 0, 300 * 1030]
    assert hp.n_terms(arr, 5) == 7 + 3 + 2 + 0 + 300
    assert hp.row_offsets(arr, 5) == [sum(sizes[:s]) for s in range(6)]
    assert int(lib.kge_row_penalty_rows_floats(arr, 5)) == sum(sizes)
    assert hp.n_terms(arr, 2) == 10 and int(lib.kge_row_penalty_rows_floats(arr, 2)) == sizes[0] + sizes[1]
    assert hp.n_terms(arr, 0) == 0 and int(lib.kge_row_penalty_rows_floats(arr, 0)) == 0
    assert int(lib.kge_row_penalty_terms(None, 0)) == 0
    for bad in (-1, 9):
        assert int(lib.kge_row_penalty_terms(arr, bad)) == -1 and int(lib.kge_row_penalty_rows_floats(arr, bad)) == -1
    assert int(lib.kge_row_penalty_terms(None, 2)) == -1
    assert int(lib.kge_row_penalty_row_offset(arr, 5, 6)) == -1 and int(lib.kge_row_penalty_row_offset(arr, 5, -1)) == -1
    assert hp.n_terms(streams_of(dict(n=-1)), 1) == -1
    # the workspace: the fp64 partials of kge_pair_loss's tree over M terms
    train = _hip.load_library()
    train.kge_pair_loss_ws_bytes.argtypes, train.kge_pair_loss_ws_bytes.restype = [ctypes.c_int64], ctypes.c_size_t
    last = 0
    for M in (1, 4, 1024, 1025, 5000, 10 ** 6, 2 ** 31 - 1):
        nb = int(lib.kge_row_penalty_ws_bytes(M))
        assert nb == int(train.kge_pair_loss_ws_bytes(M)) and nb >= last and nb % 8 == 0 and nb > 0, M
        last = nb
    for M in (0, -3, 2 ** 31, 2 ** 40):
        assert int(lib.kge_row_penalty_ws_bytes(M)) == 0, M


def fwd(lib, arr, n=1, p=3, terms=A[4], loss=A[5], acc=None, ws=A[6], ws_bytes=1 << 20):
    return int(lib.kge_row_penalty(arr, n, p, terms, loss, acc, ws, ws_bytes, None))


def bwd(lib, arr, n=1, p=3, go=A[4], rows=A[5]):
    return int(lib.kge_row_penalty_bwd(arr, n, p, go, rows, None))


@pytest.mark.parametrize('entry', [fwd, bwd])
def test_argument_checks_return_einval_before_any_launch(entry):
    lib = hp.load_library()
    ok = streams_of({})
    for p in (1, 0, 4, -2):
        assert entry(lib, ok, p=p) == EINVAL, p
    assert entry(lib, ok, n=-1) == EINVAL and entry(lib, streams_of(*[{}] * 9), n=9) == EINVAL
    assert entry(lib, None, n=1) == EINVAL
    bad = [dict(t0=None), dict(ids=None), dict(layout=hp.SPLIT), dict(layout=hp.INTERLEAVED, d=7), dict(layout=3), dict(layout=-1),
           dict(d=0), dict(d=-4), dict(ld=7), dict(n=-1), dict(n=2 ** 31), dict(layout=hp.SPLIT, t1=A[1], n=2 ** 31)]
    for s in bad:
        assert entry(lib, streams_of(s)) == EINVAL, s
        assert entry(lib, streams_of({}, {}, s), n=3) == EINVAL, s          # wherever the stream stands
    assert entry(lib, streams_of(dict(n=2 ** 30), dict(n=2 ** 30)), n=2) == EINVAL     # M = 2^31 over two streams
    if entry is fwd:
        assert fwd(lib, ok, terms=None) == EINVAL and fwd(lib, ok, loss=None) == EINVAL
        assert fwd(lib, ok, ws=None) == EINVAL and fwd(lib, ok, ws=A[6] + 4) == EINVAL
        assert fwd(lib, ok, ws_bytes=7) == EINVAL
        big = streams_of(dict(n=5000))
        assert fwd(lib, big, ws_bytes=int(lib.kge_row_penalty_ws_bytes(5000)) - 1) == EINVAL
        assert fwd(lib, streams_of(dict(n=0)), terms=None) == EINVAL            # the outputs are checked for M = 0 too
    else:
        assert bwd(lib, ok, go=None) == EINVAL and bwd(lib, ok, rows=None) == EINVAL
        # M = 0: nothing to launch, no pointer behind the descriptors is looked at
        assert bwd(lib, streams_of(dict(n=0, ids=None))) == 0 and bwd(lib, None, n=0) == 0


def test_descriptors_take_the_tables_strides_and_empty_id_vectors():
    E = torch.zeros(6, 12)
    arr, keep = hp.descriptors([(hp.REAL, E[:, :5], None, torch.tensor([1, 1, 4]), 0.5),
                                (hp.SPLIT, E[:3], E[3:], torch.zeros(0, dtype=torch.int64), 0.25)])
    assert (arr[0].ld, arr[0].d, arr[0].n, arr[0].layout, arr[0].t0) == (12, 5, 3, hp.REAL, E.data_ptr())
    assert (arr[1].ld, arr[1].d, arr[1].n, arr[1].ids, arr[1].t1) == (12, 12, 0, None, E[3:].data_ptr())
    assert arr[0].factor == 0.5
    with pytest.raises(ValueError):
        hp.descriptors([(hp.SPLIT, E[:3], E[:2], torch.tensor([0]), 1.0)])


@pytest.mark.parametrize('name', sorted(ref.zoo(4)))
def test_penalty_groups_of_every_model_class(name):
    build, (ent, rel) = ref.zoo(4)[name]
    model = build()

    def named(groups):
        by_id = {id(p): n.rsplit('.weight', 1)[0] for n, p in model.named_parameters()}
        return [(layout, tuple(by_id[id(x)] for x in tabs) if isinstance(tabs, tuple) else by_id[id(tabs)]) for layout, tabs in groups]
    got_ent, got_rel = model._penalty_groups()
    assert named(got_ent) == ent and named(got_rel) == rel
    # every entity group is an entity-indexed table, and no parameter outside an nn.Embedding is in a group
    flat = [x for _, tabs in got_ent + got_rel for x in (tabs if isinstance(tabs, tuple) else (tabs,))]
    emb = {id(m.weight) for m in model.modules() if isinstance(m, torch.nn.Embedding)}
    assert all(id(x) in emb for x in flat) and len({id(x) for x in flat}) == len(flat)
    assert {n for _, g in ent for n in (g if isinstance(g, tuple) else (g,))} == set(model._ENT_TABLES)
    # modulus=False: one REAL group per table, the same tables
    sides = LpRegularizer(p=2, weight=1.0, modulus=False)._groups(model)
    assert all(layout == hp.REAL and t1 is None for side in sides for layout, t0, t1 in side)
    assert [id(t0) for side in sides for _, t0, _ in side] == [id(x) for x in flat]
    for n in model._DENSE_GRAD_TABLES:
        assert any(x is getattr(model, n).weight for x in flat), n


def test_the_base_default_splits_embedding_tables_by_ent_tables():
    from torchkge_amd.models.interfaces import Model

    class Toy(Model):
        _ENT_TABLES = ('a',)

        def __init__(self):
            super().__init__(4, 2)
            self.a, self.b = torch.nn.Embedding(4, 3), torch.nn.Embedding(2, 3)
            self.lin = torch.nn.Linear(3, 1)

        def _tables(self):
            return [self.a.weight, self.b.weight, self.lin.weight]
    m = Toy()
    ent, rel = m._penalty_groups()
    assert [(layout, x is m.a.weight) for layout, x in ent] == [(hp.REAL, True)]
    assert [(layout, x is m.b.weight) for layout, x in rel] == [(hp.REAL, True)]


@pytest.mark.parametrize('layout', [ref.REAL, ref.SPLIT, ref.INTERLEAVED])
@pytest.mark.parametrize('p', [2, 3])
def test_the_yardsticks_closed_form_gradient_matches_central_differences_and_is_zero_at_zero(layout, p):
    g = torch.Generator().manual_seed(5)
    t0 = torch.randn(3, 6, generator=g)
    t1 = torch.randn(3, 6, generator=g) if layout == ref.SPLIT else None
    grads = ref.row_gradients(layout, p, t0, t1)
    grads = grads if layout == ref.SPLIT else (grads,)
    for which, (t, got) in enumerate(zip((t0, t1), grads)):
        for i, k in ((0, 0), (1, 3), (2, 5)):
            h = 1e-4
            hi, lo = [x if x is None else x.double().clone() for x in (t0, t1)], [x if x is None else x.double().clone() for x in (t0, t1)]
            hi[which][i, k] += h
            lo[which][i, k] -= h
            fd = (ref.row_power_sums(layout, p, *hi)[i] - ref.row_power_sums(layout, p, *lo)[i]) / (2 * h)
            assert abs(fd - got[i, k]) <= 1e-6 * max(1.0, abs(fd)), (which, i, k)
    z = torch.zeros(2, 6)
    gz = ref.row_gradients(layout, p, z, z if layout == ref.SPLIT else None)
    for x in (gz if layout == ref.SPLIT else (gz,)):
        assert torch.equal(x, torch.zeros(2, 6, dtype=torch.float64))
    assert torch.equal(ref.row_power_sums(layout, p, z, z if layout == ref.SPLIT else None), torch.zeros(2, dtype=torch.float64))


def test_regularizer_arguments():
    for p in (1, 4, 2.5, 0):
        with pytest.raises(ValueError):
            LpRegularizer(p=p, weight=0.1)
    r = LpRegularizer(p=2, weight=0.1)
    assert (r.p, r.weight, r.relation_weight, r.modulus) == (2, 0.1, 0.1, True)
    n3 = N3Regularizer(0.05, relation_weight=0.2)
    assert isinstance(n3, LpRegularizer) and (n3.p, n3.weight, n3.relation_weight, n3.modulus) == (3, 0.05, 0.2, True)
    assert list(inspect.signature(LpRegularizer.__init__).parameters) == ['self', 'p', 'weight', 'relation_weight', 'modulus']
    assert list(inspect.signature(LpRegularizer.__call__).parameters) == ['self', 'model', 'entity_ids', 'relation_ids', 'acc']
    # a row-sharded model raises before anything is launched
    build, _ = ref.zoo(4)['DistMult']
    model = build().shard_entities_(0, 10)
    with pytest.raises(RuntimeError, match='whole entity tables'):
        n3(model, (torch.tensor([1]),), (torch.tensor([0]),))


def test_the_trainers_attribute_is_none_by_default_and_the_constructors_are_unchanged():
    for cls in (Trainer, OneVsAllTrainer, KvsAllTrainer):
        assert cls.regularizer is None and 'regularizer' not in inspect.signature(cls.__init__).parameters, cls
    assert list(inspect.signature(Trainer.__init__).parameters) == [
        'self', 'model', 'criterion', 'kg_train', 'n_epochs', 'batch_size', 'optimizer', 'sampling_type', 'use_cuda', 'fused',
        'sync_free', 'sampler', 'verbose', 'n_neg']
    for cls in (OneVsAllTrainer, KvsAllTrainer):
        assert list(inspect.signature(cls.__init__).parameters) == [
            'self', 'model', 'kg_train', 'n_epochs', 'batch_size', 'optimizer', 'label_smoothing', 'side', 'use_cuda', 'sync_free',
            'verbose']
    assert Trainer.grouped_forward is False
