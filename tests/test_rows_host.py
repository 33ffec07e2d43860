"""CPU-only tests of row gradients: the switch (torchkge_amd/rowgrad.py), the exports and ctypes signatures of
include/kge_hip_rows.h, the untouched include/kge_hip.h, the workspace bound, the optimizers' argument checks with the
dense-gradient error, and split_parameters on one model of each family."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import pytest
import torch

from tests.helpers import ROOT
from tests.test_deterministic_host import KGE_HIP_H_SHA256

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_rows, optim, rowgrad

HEADER = os.path.join(ROOT, 'include', 'kge_hip_rows.h')
ENTRIES = ('kge_rows_coalesce', 'kge_row_sgd', 'kge_row_adagrad', 'kge_row_adam')
QUERIES = ('kge_rows_coalesce_ws_bytes', 'kge_row_update_max_waves')


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def prototypes():
    return dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', header_text(), flags=re.S))


# ---------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------
def test_switch_defaults_off_and_follows_the_environment():
    code = 'import torchkge_amd as tk; print(tk.is_row_gradients())'
    env = {k: v for k, v in os.environ.items() if k != 'KGE_ROW_GRADIENTS'}
    run = lambda e: subprocess.check_output([sys.executable, '-c', code], cwd=ROOT, env=e, text=True).strip()   # noqa: E731
    assert run(env) == 'False'
    assert run(dict(env, KGE_ROW_GRADIENTS='1')) == 'True'
    assert run(dict(env, KGE_ROW_GRADIENTS='0')) == 'False'


def test_switch_set_get_nesting_and_restore_after_an_exception():
    assert tk.set_row_gradients is rowgrad.set_row_gradients and tk.row_gradients is rowgrad.row_gradients
    assert tk.is_row_gradients is rowgrad.is_row_gradients
    start = tk.is_row_gradients()
    try:
        tk.set_row_gradients(False)
        assert tk.is_row_gradients() is False
        tk.set_row_gradients(True)
        assert tk.is_row_gradients() is True
        tk.set_row_gradients(False)
        with tk.row_gradients():
            assert tk.is_row_gradients()
            with tk.row_gradients(False):
                assert not tk.is_row_gradients()
                with tk.row_gradients(True):
                    assert tk.is_row_gradients()
                assert not tk.is_row_gradients()
            assert tk.is_row_gradients()
        assert not tk.is_row_gradients()
        with pytest.raises(ValueError):
            with tk.row_gradients():
                assert tk.is_row_gradients()
                raise ValueError('x')
        assert not tk.is_row_gradients()
        ctx = tk.row_gradients()                # one instance entered twice
        with ctx:
            with ctx:
                assert tk.is_row_gradients()
            assert tk.is_row_gradients()
        assert not tk.is_row_gradients()

        @tk.row_gradients()
        def inside():
            return tk.is_row_gradients()
        assert inside() is True and not tk.is_row_gradients()
        tk.set_row_gradients(True)
        with tk.row_gradients(False):
            assert not tk.is_row_gradients()
        assert tk.is_row_gradients()            # restored to the state before, not to off
    finally:
        tk.set_row_gradients(start)


def test_switch_is_independent_of_the_deterministic_mode():
    assert not tk.is_row_gradients() and not tk.is_deterministic()
    with tk.row_gradients():
        assert not tk.is_deterministic()
    with tk.deterministic():
        assert not tk.is_row_gradients()


# ---------------------------------------------------------------------------
# the header and its binding
# ---------------------------------------------------------------------------
def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_rows.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(ENTRIES) | set(QUERIES)
    assert set(ENTRIES) == set(_hip_rows._SIGNATURES) and set(_hip_rows._WS_SIZES) == {QUERIES[0]}
    assert set(prototypes()) == set(ENTRIES) | {QUERIES[1]}
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    for name in declared:
        assert hasattr(lib, name), name
    from torchkge_amd.csrc import build as hb
    assert 'row_optim.hip' in hb.SOURCES and '-ffp-contract=off' in hb.FLAGS
    assert any(h.endswith('kge_hip_rows.h') for h in hb.HEADERS)
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    # the source has no atomic of its own, and the ordered level kernels exist once: it calls the entry, it has no copy
    code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, 'row_optim.hip')).read())
    assert not re.search(r'atomic', code, flags=re.I)
    assert 'kge_segment_sum_ordered(' in code and 'segment_sum_ordered_kernel' not in code


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
        if 'int' in t or 'int32_t' in t:
            return ctypes.c_int
        raise AssertionError('unparsed parameter: %r' % param)
    for name, args in _hip_rows._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            assert a is kind(prm), (name, prm)
    lib = _hip_rows.load_library()
    for name, args in _hip_rows._SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    f = lib.kge_rows_coalesce_ws_bytes
    assert f.argtypes == [ctypes.c_int64, ctypes.c_int] and f.restype is ctypes.c_size_t
    assert re.search(r'\bsize_t\s+kge_rows_coalesce_ws_bytes\s*\(\s*int64_t \w+\s*,\s*int \w+\s*\)\s*;', open(HEADER).read())
    assert protos['kge_row_update_max_waves'].strip() == 'void'
    assert lib.kge_row_update_max_waves.argtypes == [] and lib.kge_row_update_max_waves.restype is ctypes.c_int
    assert _hip_rows.max_waves() >= 1024 and _hip_rows.max_waves() % 4 == 0


def test_the_main_header_and_its_abi_are_untouched():
    assert _hip.ABI_VERSION == 33 and _hip.load_library().kge_abi_version() == 33
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    assert hashlib.sha256(raw).hexdigest() == KGE_HIP_H_SHA256
    for name in ENTRIES + QUERIES:
        assert name.encode() not in raw
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


def test_workspace_bound_is_zero_for_bad_arguments_and_monotone():
    lib = _hip_rows.load_library()       # (a process without a GPU: the size query launches nothing)
    f = lib.kge_rows_coalesce_ws_bytes
    assert [int(f(M, 64)) for M in (-1, 0, 1 << 31)] == [0, 0, 0]
    assert int(f(5, 0)) == 0 and int(f(5, -3)) == 0
    for d in (1, 7, 64, 200, 1024, 1030):
        prev = 0
        for M in list(range(1, 300)) + [1000, 2053, 32768, 65536, 65537, 131072, 1 << 22]:
            b = int(f(M, d))
            assert b > 0 and b >= prev, (M, d)
            prev = b
    for M in (1, 33, 2053, 65536):
        sizes = [int(f(M, d)) for d in list(range(1, 1100)) + [2048, 4096]]
        assert sizes == sorted(sizes)
        assert int(f(M, 1024)) == int(f(M, 5000))       # wider rows go in column chunks of 1024
        # the order, the ranks and the ordered reduction's own workspace all fit
        from torchkge_amd import _hip_det
        assert int(f(M, 64)) >= 16 * M + _hip_det.ws_bytes(M, 64)
    assert _hip_rows.ws_bytes(2053, 8) == int(f(2053, 8)) and (2053, 8) in _hip_rows._WS_BYTES


# ---------------------------------------------------------------------------
# the optimizers on the host: arguments, and what they refuse
# ---------------------------------------------------------------------------
def test_optimizer_argument_validation():
    p = [torch.nn.Parameter(torch.zeros(4, 3))]
    for cls in (optim.RowSGD, optim.RowAdagrad, optim.RowAdam):
        assert issubclass(cls, torch.optim.Optimizer)
        with pytest.raises(ValueError, match='learning rate'):
            cls(p, lr=-0.1)
        with pytest.raises(ValueError):
            cls([], lr=0.1)                                 # torch's own: an empty parameter list
        assert cls.zero_grad is torch.optim.Optimizer.zero_grad
    with pytest.raises(ValueError, match='lr_decay'):
        optim.RowAdagrad(p, lr=0.1, lr_decay=-1)
    with pytest.raises(ValueError, match='epsilon'):
        optim.RowAdagrad(p, lr=0.1, eps=-1e-3)
    with pytest.raises(ValueError, match='initial_accumulator_value'):
        optim.RowAdagrad(p, lr=0.1, initial_accumulator_value=-1)
    with pytest.raises(ValueError, match='epsilon'):
        optim.RowAdam(p, lr=0.1, eps=0.0)
    for betas in ((1.0, 0.9), (0.9, 1.0), (-0.1, 0.9)):
        with pytest.raises(ValueError, match='beta'):
            optim.RowAdam(p, lr=0.1, betas=betas)
    o = optim.RowAdagrad(p, lr=0.5)
    assert o.defaults == dict(lr=0.5, lr_decay=0, eps=1e-10, initial_accumulator_value=0)
    assert optim.RowAdam(p, lr=0.5).defaults == dict(lr=0.5, betas=(0.9, 0.999), eps=1e-8)
    assert optim.RowSGD(p, lr=0.5).defaults == dict(lr=0.5)


@pytest.mark.parametrize('cls', ['RowSGD', 'RowAdagrad', 'RowAdam'])
def test_a_dense_gradient_raises_and_names_the_way_out(cls):
    p = torch.nn.Parameter(torch.ones(4, 3))
    o = getattr(optim, cls)([p], lr=0.1)
    o.step()                                                # no gradient at all: nothing to do
    p.grad = torch.ones(4, 3)
    with pytest.raises(RuntimeError, match='dense gradient.*stock torch.optim optimizer'):
        o.step()
    assert torch.equal(p.detach(), torch.ones(4, 3)) and not o.state[p]
    # a sparse gradient of a parameter that is not on the GPU is refused as well, before any launch
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1, 1]]), torch.ones(2, 3), (4, 3))
    with pytest.raises(RuntimeError, match='on the GPU'):
        o.step()
    assert torch.equal(p.detach(), torch.ones(4, 3))
    o.zero_grad()
    assert p.grad is None


def test_coalesce_rows_refuses_what_is_not_a_row_gradient():
    with pytest.raises(RuntimeError, match='sparse COO'):
        optim.coalesce_rows(torch.ones(4, 3))
    with pytest.raises(RuntimeError, match='sparse COO'):       # both dimensions sparse: the rows are not dense
        optim.coalesce_rows(torch.sparse_coo_tensor(torch.tensor([[1], [2]]), torch.ones(1), (4, 3)))


def test_split_parameters_on_one_model_of_each_family():
    cases = [
        (tk.TransEModel(8, 11, 3, 'L2'), ['ent_emb', 'rel_emb'], []),
        (tk.TransHModel(8, 11, 3), ['ent_emb', 'rel_emb', 'norm_vect'], []),
        (tk.TransDModel(8, 6, 11, 3), ['ent_emb', 'rel_emb', 'ent_proj_vect', 'rel_proj_vect'], []),
        (tk.TransRModel(8, 6, 11, 3), ['ent_emb', 'rel_emb'], ['proj_mat']),
        (tk.TorusEModel(8, 11, 3, 'torus_L2'), ['ent_emb', 'rel_emb'], []),
        (tk.DistMultModel(8, 11, 3), ['ent_emb', 'rel_emb'], []),
        (tk.ComplExModel(8, 11, 3), ['re_ent_emb', 'im_ent_emb', 're_rel_emb', 'im_rel_emb'], []),
        (tk.RESCALModel(4, 11, 3), ['ent_emb'], ['rel_mat']),
        (tk.HolEModel(8, 11, 3), ['ent_emb', 'rel_emb'], []),
        (tk.AnalogyModel(8, 11, 3), ['sc_ent_emb', 're_ent_emb', 'im_ent_emb', 'sc_rel_emb', 're_rel_emb', 'im_rel_emb'], []),
        (tk.ConvKBModel(8, 2, 11, 3), ['ent_emb', 'rel_emb'], ['convlayer.0', 'convlayer.0', 'output.0', 'output.0']),
    ]
    for model, want_row, want_dense in cases:
        names = {id(p): n.rsplit('.', 1)[0] for n, p in model.named_parameters()}
        row, dense = optim.split_parameters(model)
        assert sorted(names[id(p)] for p in row) == sorted(want_row), type(model).__name__
        assert sorted(names[id(p)] for p in dense) == sorted(want_dense), type(model).__name__
        assert len(row) + len(dense) == len(list(model.parameters()))
        assert all(p.dim() == 2 for p in row)


def test_names_the_engine_leaves_out_still_raise():
    from torchkge_amd import utils
    for mod, name in ((utils, 'Trainer'), (utils, 'TrainDataLoader')):
        assert not hasattr(mod, name)
        with pytest.raises(AttributeError, match='does not provide'):
            getattr(mod, name)
    for name in ('set_row_gradients', 'is_row_gradients', 'row_gradients'):
        assert callable(getattr(tk, name))
    assert sorted(optim.__all__) == ['RowAdagrad', 'RowAdam', 'RowSGD', 'coalesce_rows', 'split_parameters']
