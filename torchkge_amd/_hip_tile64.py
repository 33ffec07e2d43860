# -*- coding: utf-8 -*-
"""What the ctypes bindings of the all-candidates criteria share (``_hip_xent``, ``_hip_bce``; the 64 x 64 skeleton of
csrc/lp_tile64.h): the constants their headers publish, the library handle with a header's prototypes bound, the
per-shape workspace, and the gradient groups of a backward call with their ``(pointer, stride)`` arguments.  Nothing
here synchronises or reads back."""
import ctypes

import torch

from . import _hip
from ._hip import _i64, _int, _p

_size = ctypes.c_size_t
_f32 = ctypes.c_float
# the constants of both headers (KGE_XENT_* / KGE_BCE_*: csrc/lp_tile64.h holds them equal)
BM, BN = 64, 64                 # queries per row panel, candidates per tile
MIN_TILES_PER_CHUNK = 4
MAX_CHUNKS = 32
MAX_K = 1024
KSLICE = 512


def load_library(signatures, ws_sizes, chunks_name):
    """The handle of _hip.load_library() with the argtypes of one criterion's header bound."""
    lib = _hip.bind(signatures, ws_sizes, (_i64, _i64, _int, _int), _size)
    f = getattr(lib, chunks_name)
    f.argtypes, f.restype = [_i64], _int
    return lib


def ws_bytes(cache, load_library, name, B, N, K0, K1):
    """A criterion's workspace-size query ``name`` of ``load_library()``: host arithmetic, cached per shape in the
    criterion's ``cache`` (a hit does not touch the library)."""
    key = (B, N, K0, K1)
    nb = cache.get(key)
    if nb is None:
        nb = cache[key] = int(getattr(load_library(), name)(B, N, K0, K1))
    return nb


def workspace(prob, ws_bytes_of):
    d = prob.desc
    return torch.empty(max(ws_bytes_of(int(d.B), int(d.N), int(d.K0), int(d.K1)), 16), dtype=torch.uint8, device=prob.device)


def grad_groups(prob, want_queries, want_tables):
    """``(dA, dT, launch)``: per group the list of one float32 gradient per segment (queries: (B, K), tables: (N, K)), or
    None when it is not wanted.  ``launch`` is False when no kernel would write them -- nothing wanted, or B == 0 -- and
    they are zero-filled here instead."""
    d, dev = prob.desc, prob.device
    segs = [int(d.K0)] + ([int(d.K1)] if d.K1 else [])
    dA = [torch.empty(prob.B, k, dtype=torch.float32, device=dev) for k in segs] if want_queries else None
    dT = [torch.empty(prob.N, k, dtype=torch.float32, device=dev) for k in segs] if want_tables else None
    launch = (want_queries or want_tables) and prob.B != 0
    if not launch:
        for grp in (dA, dT):
            for x in grp or ():
                x.zero_()
    return dA, dT, launch


def group_args(*groups):
    """The ``pointer, stride`` pairs of the entries' two segments per gradient group; null for what is absent."""
    out = []
    for grp in groups:
        for j in range(2):
            x = grp[j] if grp is not None and j < len(grp) else None
            out += [_p(x), 0 if x is None else x.stride(0)]
    return out
