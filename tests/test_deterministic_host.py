"""CPU-only tests of the deterministic training mode: the exports and ctypes signatures of include/kge_hip_det.h, the
untouched include/kge_hip.h, the workspace bound (host arithmetic, no device), the level plan under the host sanitizers
as a stand-alone program, and the semantics of the switch (torchkge_amd/determinism.py)."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from tests.helpers import ROOT

import torchkge_amd as tk
from torchkge_amd import _hip, _hip_det, determinism

HEADER = os.path.join(ROOT, 'include', 'kge_hip_det.h')
NEW = ('kge_segment_sum_ordered',)
WS = ('kge_segment_sum_ordered_ws_bytes',)
# sha256 of include/kge_hip.h as the parent commit has it: nothing of it changes for this entry point
KGE_HIP_H_SHA256 = '1d27fe190e8113e167cb0ae9d5108c0a08ab6569765f853cc884e29f00462b4c'


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def prototypes():
    return dict(re.findall(r'\bint\s+(kge_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', header_text(), flags=re.S))


def test_library_exports_every_symbol_the_header_declares():
    lib = _hip_det.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(NEW) | set(WS)
    assert set(NEW) == set(_hip_det._SIGNATURES) == set(prototypes()) and set(WS) == set(_hip_det._WS_SIZES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    assert declared <= set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    for name in declared:
        assert hasattr(lib, name), name
    from torchkge_amd.csrc import build as hb
    assert 'segment_sum_ordered.hip' in hb.SOURCES and 'segment_levels.h' in hb.HEADERS
    assert 'segment_sum_rows.hip' in hb.SOURCES
    assert any(h.endswith('kge_hip_det.h') for h in hb.HEADERS)
    for h in hb.HEADERS:
        assert os.path.exists(os.path.join(hb.HERE, h)), h
    # no float atomic in the source of the ordered reduction (its contract), and none of its own
    src = open(os.path.join(hb.HERE, 'segment_sum_ordered.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert not re.search(r'atomic', code, flags=re.I)


def test_ctypes_signatures_match_the_header_prototypes():
    """Same number of parameters, pointers as void*, int64_t as c_int64, size_t as c_size_t (the checker of
    tests/test_triplet_host.py)."""
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
    for name, args in _hip_det._SIGNATURES.items():
        params = protos[name].split(',')
        assert len(params) == len(args), (name, len(params), len(args))
        for prm, a in zip(params, args):
            k = kind(prm)
            if k is ctypes.c_int:
                assert a in (ctypes.c_int, ctypes.c_int32), (name, prm)
            else:
                assert a is k, (name, prm)
    lib = _hip_det.load_library()
    for name, args in _hip_det._SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int
    for name in WS:
        assert getattr(lib, name).argtypes == [ctypes.c_int64, ctypes.c_int] and getattr(lib, name).restype is ctypes.c_size_t
        assert re.search(r'\bsize_t\s+%s\s*\(\s*int64_t \w+\s*,\s*int \w+\s*\)\s*;' % name, open(HEADER).read())


def test_the_main_header_and_its_abi_are_untouched():
    assert _hip.ABI_VERSION == 33 and _hip.load_library().kge_abi_version() == 33
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    assert hashlib.sha256(raw).hexdigest() == KGE_HIP_H_SHA256
    for name in NEW + WS:
        assert name.encode() not in raw
        assert name not in _hip.EXPORTED_SYMBOLS and name not in _hip._SIGNATURES


def test_workspace_bound_is_host_arithmetic_monotone_and_zero_only_without_entries():
    lib = _hip_det.load_library()       # (a process without a GPU: the size query makes no device call)
    f = lib.kge_segment_sum_ordered_ws_bytes
    assert [int(f(M, 64)) for M in (-1, 0)] == [0, 0]
    assert int(f(5, 0)) == 0 and int(f(5, 1025)) == 0          # a d the entry refuses has no workspace
    for d in (1, 63, 64, 200, 1024):
        prev = 0
        for M in list(range(1, 300)) + [1000, 2053, 32768, 65536, 65537, 1 << 22]:
            b = int(f(M, d))
            assert b >= 16 and b >= prev, (M, d)
            prev = b
    for M in (1, 33, 2053, 65536):
        sizes = [int(f(M, d)) for d in range(1, 1025)]
        assert sizes == sorted(sizes)
    # levels 2053 -> 130 -> 10: 140 slots of a key and a row each; about M / 16 rows for a large M
    assert int(f(2053, 8)) == 140 * (8 + 4 * 8)
    assert int(f(1 << 22, 512)) < ((1 << 22) // 14) * (8 + 4 * 512)
    assert _hip_det.ws_bytes(2053, 8) == 140 * 40 and (2053, 8) in _hip_det._WS_BYTES


def test_level_plan_under_the_host_sanitizers(tmp_path):
    """The level sizes and workspace offsets live in a host header (csrc/segment_levels.h): a stand-alone program walks
    them over a real buffer under AddressSanitizer + UBSan."""
    cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'det_levels')
    static = [] if cxx == 'clang++' else ['-static-libasan', '-static-libubsan']     # (clang links its runtimes statically)
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all'] + static +
                          [os.path.join(ROOT, 'tests', 'det_levels_main.cpp'), '-o', exe])
    out = subprocess.check_output([exe], text=True)
    assert out.strip() == 'level plan: ok'


def test_switch_defaults_off_and_follows_the_environment():
    code = 'import torchkge_amd as tk; print(tk.is_deterministic())'
    env = {k: v for k, v in os.environ.items() if k != 'KGE_DETERMINISTIC'}
    run = lambda e: subprocess.check_output([sys.executable, '-c', code], cwd=ROOT, env=e, text=True).strip()   # noqa: E731
    assert run(env) == 'False'
    assert run(dict(env, KGE_DETERMINISTIC='1')) == 'True'
    assert run(dict(env, KGE_DETERMINISTIC='0')) == 'False'


def test_switch_set_get_nesting_and_restore_after_an_exception():
    assert tk.set_deterministic is determinism.set_deterministic and tk.deterministic is determinism.deterministic
    assert not torch.are_deterministic_algorithms_enabled()
    start = tk.is_deterministic()
    try:
        tk.set_deterministic(False)
        assert tk.is_deterministic() is False
        tk.set_deterministic(True)
        assert tk.is_deterministic() is True
        tk.set_deterministic(False)
        with tk.deterministic():
            assert tk.is_deterministic()
            with tk.deterministic(False):
                assert not tk.is_deterministic()
                with tk.deterministic(True):
                    assert tk.is_deterministic()
                assert not tk.is_deterministic()
            assert tk.is_deterministic()
        assert not tk.is_deterministic()
        with pytest.raises(ValueError):
            with tk.deterministic():
                assert tk.is_deterministic()
                raise ValueError('x')
        assert not tk.is_deterministic()
        ctx = tk.deterministic()                # one instance entered twice
        with ctx:
            with ctx:
                assert tk.is_deterministic()
            assert tk.is_deterministic()
        assert not tk.is_deterministic()

        @tk.deterministic()
        def inside():
            return tk.is_deterministic()
        assert inside() is True and not tk.is_deterministic()
        tk.set_deterministic(True)
        with tk.deterministic(False):
            assert not tk.is_deterministic()
        assert tk.is_deterministic()            # restored to the state before, not to off
    finally:
        tk.set_deterministic(start)


def test_torchs_flag_alone_turns_the_mode_on():
    start = tk.is_deterministic()
    tk.set_deterministic(False)
    try:
        for warn_only in (False, True):
            torch.use_deterministic_algorithms(True, warn_only=warn_only)
            try:
                assert tk.is_deterministic()
                with tk.deterministic(False):       # the package switch off does not override torch's flag
                    assert tk.is_deterministic()
            finally:
                torch.use_deterministic_algorithms(False)
            assert not tk.is_deterministic()
    finally:
        tk.set_deterministic(start)


def test_names_the_engine_leaves_out_still_raise():
    """The switch adds three names at the top level and nothing else: what the engine leaves out still says so."""
    from torchkge_amd import utils
    for mod, name in ((utils, 'Trainer'), (utils, 'TrainDataLoader'), (tk, 'TripletClassificationEvaluator'),
                      (tk, 'PositionalNegativeSampler'), (tk, 'RelationInference')):
        assert not hasattr(mod, name)
        with pytest.raises(AttributeError, match='does not provide'):
            getattr(mod, name)
    assert not hasattr(tk, 'no_such_name')
    for name in ('set_deterministic', 'is_deterministic', 'deterministic'):
        assert callable(getattr(tk, name))
