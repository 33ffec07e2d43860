"""CPU-only tests of filtered negative sampling (include/kge_hip_filtered.h): the exports and ctypes signatures, the
KGE_EINVAL table of both entries on never-dereferenced aligned addresses (every refusal happens before a launch), the
pure-Python restatement of the seven steps (tests/filtered_ref.py) against brute-force enumeration for EVERY
(n_ent <= 12, list, replaced entity), the index source of FilteredNegativeSampler (the train child's own triples, not the
parent's filter sets) and its parameter lists."""
import ctypes
import inspect
import itertools
import os
import re
import subprocess

import torch

from tests import filtered_ref as ref
from tests.helpers import ROOT

from torchkge_amd import _hip, _hip_filtered as hf

HEADER = os.path.join(ROOT, 'include', 'kge_hip_filtered.h')
ENTRIES = ('kge_filtered_corrupt', 'kge_triples_known')
EINVAL = -1


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_library_exports_exactly_the_symbols_the_header_declares_and_the_build_lists_the_file():
    lib = hf.load_library()
    declared = set(re.findall(r'\b(kge_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == set(ENTRIES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _hip.LIB_PATH], text=True)
    exported = set(re.findall(r' T (kge_[a-z0-9_]+)', out))
    assert declared <= exported
    # exactly: the new translation unit exports nothing that the header does not declare
    unit = open(os.path.join(ROOT, 'torchkge_amd', 'csrc', 'filtered_corrupt.hip')).read()
    assert set(re.findall(r'extern "C"[^(]*?\b(kge_[a-z0-9_]+)\s*\(', unit)) == declared
    for name in declared:
        assert hasattr(lib, name), name
    from torchkge_amd.csrc import build as hb
    assert 'filtered_corrupt.hip' in hb.SOURCES and 'filtered_corrupt.hip' not in hb.EXTRA_FLAGS       # the common flags
    assert any(h.endswith('kge_hip_filtered.h') for h in hb.HEADERS)
    # integer work only: no atomic and no float in the translation unit
    code = re.sub(r'//[^\n]*', '', open(os.path.join(hb.HERE, 'filtered_corrupt.hip')).read())
    assert not re.search(r'atomic|\bfloat\b|\bdouble\b', code, flags=re.I)


def test_kge_hip_h_does_not_hold_the_new_names_and_the_abi_version_is_33():
    lib = hf.load_library()
    raw = open(os.path.join(ROOT, 'include', 'kge_hip.h'), 'rb').read()
    for name in ENTRIES:
        assert name.encode() not in raw and name not in _hip._SIGNATURES
    assert b'kge_hip_filtered' not in raw
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
    assert set(protos) == set(hf._SIGNATURES) == set(ENTRIES)
    lib = hf.load_library()
    for name, args in hf._SIGNATURES.items():
        params = protos[name].split(',')
        assert [kind(p) for p in params] == args, name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int


# ---------------------------------------------------------------------------
# the refusals: every one before a launch, on addresses nobody reads
# ---------------------------------------------------------------------------
A = [4096 * (i + 1) for i in range(16)]     # 16-byte aligned, never dereferenced
CORRUPT_POINTERS = ('h', 't', 'mask', 'draws', 'tail_lo', 'tail_hi', 'tail_targets', 'head_lo', 'head_hi', 'head_targets',
                    'neg_h', 'neg_t')


def corrupt(lib, B=4, n_neg=3, n_ent=37, exhausted=A[12], **null):
    p = {name: A[i] for i, name in enumerate(CORRUPT_POINTERS)}
    p.update(null)
    return int(lib.kge_filtered_corrupt(p['h'], p['t'], B, n_neg, p['mask'], p['draws'], p['tail_lo'], p['tail_hi'],
                                        p['tail_targets'], p['head_lo'], p['head_hi'], p['head_targets'], n_ent, p['neg_h'],
                                        p['neg_t'], exhausted, None))


def known(lib, n=4, n_keys=5, key_span=1 << 31, keys=A[0], offsets=A[1], targets=A[2], key1=A[3], key2=A[4], value=A[5],
          out=A[6]):
    return int(lib.kge_triples_known(keys, n_keys, offsets, targets, key_span, key1, key2, value, n, out, None))


def test_filtered_corrupt_argument_checks_return_einval_before_any_launch():
    lib = hf.load_library()
    assert corrupt(lib, B=-1) == EINVAL
    assert corrupt(lib, n_neg=0) == EINVAL and corrupt(lib, n_neg=-2) == EINVAL
    assert corrupt(lib, n_ent=0) == EINVAL and corrupt(lib, n_ent=-5) == EINVAL
    assert corrupt(lib, n_ent=1 << 31) == EINVAL and corrupt(lib, n_ent=1 << 40) == EINVAL
    assert corrupt(lib, B=1 << 16, n_neg=1 << 15) == EINVAL             # B * n_neg = 2^31
    assert corrupt(lib, B=(1 << 31) - 1, n_neg=2) == EINVAL
    assert corrupt(lib, B=1 << 31, n_neg=1) == EINVAL
    for name in CORRUPT_POINTERS:
        assert corrupt(lib, **{name: None}) == EINVAL, name
    # B = 0 launches nothing and looks at no pointer, whatever n_neg is
    none = {name: None for name in CORRUPT_POINTERS}
    assert corrupt(lib, B=0, exhausted=None, **none) == 0
    assert corrupt(lib, B=0, n_neg=0, exhausted=None, **none) == 0
    assert corrupt(lib, B=0) == 0


def test_triples_known_argument_checks_return_einval_before_any_launch():
    lib = hf.load_library()
    assert known(lib, n=-1) == EINVAL and known(lib, n=1 << 31) == EINVAL
    assert known(lib, n_keys=-1) == EINVAL
    assert known(lib, key_span=0) == EINVAL and known(lib, key_span=-7) == EINVAL
    for name in ('key1', 'key2', 'value', 'out'):
        assert known(lib, **{name: None}) == EINVAL, name
    for name in ('keys', 'offsets', 'targets'):
        assert known(lib, **{name: None}) == EINVAL, name
    # n = 0 launches nothing and looks at no pointer
    assert known(lib, n=0, keys=None, offsets=None, targets=None, key1=None, key2=None, value=None, out=None) == 0
    assert known(lib, n=0) == 0


# ---------------------------------------------------------------------------
# the rule, restated, against brute force
# ---------------------------------------------------------------------------
def test_restatement_agrees_with_brute_force_for_every_small_case():
    """Every n_ent <= 12, every list L (subset of the entities), every replaced entity x: draws 0 .. c - 1 give the free
    entities in ascending order, draw c wraps to the first, the top draw and a negative bit pattern reduce modulo c, and
    c = 0 is exhausted with x unchanged."""
    cases = 0
    for n_ent in range(1, 13):
        ents = range(n_ent)
        for m in range(n_ent + 1):
            for L in itertools.combinations(ents, m):
                L = list(L)
                for x in ents:
                    free = ref.free_entities(x, L, n_ent)
                    c = len(free)
                    cases += 1
                    if c == 0:
                        assert ref.replace(x, L, 0, n_ent) == (x, 1) and ref.replace(x, L, 12345, n_ent) == (x, 1)
                        continue
                    assert [ref.replace(x, L, d, n_ent) for d in range(c)] == [(e, 0) for e in free], (n_ent, L, x)
                    assert ref.replace(x, L, c, n_ent) == (free[0], 0)
                    assert ref.replace(x, L, (1 << 62) - 1, n_ent) == (free[((1 << 62) - 1) % c], 0)
                    assert ref.replace(x, L, -3, n_ent) == (free[((1 << 64) - 3) % c], 0)      # read as uint64
    assert cases == sum(n * 2 ** n for n in range(1, 13))


def test_batch_restatement_uses_tile_order_and_the_side_of_the_mask():
    h, t = [3, 0], [1, 4]
    tails, heads = [[1, 2], []], [[3], [0, 1, 2, 3]]
    #        k = 0: head of fact 0, tail of fact 1      k = 1: tail of fact 0, head of fact 1 (one entity free: 4)
    mask, draws = [1, 0, 0, 1], [0, 1, 2, 7]
    nh, nt, ex = ref.corrupt(h, t, 2, mask, draws, tails, heads, 5)
    assert (nh, nt, ex) == ([0, 0, 3, 4], [1, 1, 4, 4], [0, 0, 0, 0])
    # fact 1's head list with 4 added: every entity is a known head, the position is exhausted and keeps the fact
    nh, nt, ex = ref.corrupt(h, t, 2, mask, draws, tails, [[3], [0, 1, 2, 3, 4]], 5)
    assert (nh[3], nt[3], ex[3]) == (0, 4, 1) and ex[:3] == [0, 0, 0]
    index = {(0, 1): {2, 3}, (4, 0): [1]}
    assert ref.known(index, [0, 0, 4, 4, 2], [1, 1, 0, 1, 0], [2, 4, 1, 1, 2]) == [1, 0, 1, 0, 0]


# ---------------------------------------------------------------------------
# the sampler's host side
# ---------------------------------------------------------------------------
def parent_graph():
    import torchkge_amd as tk
    g = torch.Generator().manual_seed(11)
    n_ent, n_rel, n = 30, 3, 400
    trip = torch.stack([torch.randint(0, n_ent, (n,), generator=g), torch.randint(0, n_ent, (n,), generator=g),
                        torch.randint(0, n_rel, (n,), generator=g)], 1)
    trip = torch.unique(trip, dim=0)
    trip = trip[torch.randperm(trip.shape[0], generator=g)]
    return tk.KnowledgeGraph(kg={'heads': trip[:, 0].contiguous(), 'tails': trip[:, 1].contiguous(),
                                 'relations': trip[:, 2].contiguous()},
                             ent2ix={i: i for i in range(n_ent)}, rel2ix={i: i for i in range(n_rel)})


def index_as_dict(ix):
    keys, off, tg = ix.keys.tolist(), ix.offsets.tolist(), ix.targets.tolist()
    span = 1 << 31
    return {(k // span, k % span): set(tg[off[q]:off[q + 1]]) for q, k in enumerate(keys)}


def test_sampler_on_a_split_child_indexes_only_the_childs_own_triples():
    from torchkge_amd.sampling import FilteredNegativeSampler
    kg = parent_graph()
    n = kg.n_facts
    train, val, test = kg.split_kg(sizes=(n - 120, 60, 60))
    sampler = FilteredNegativeSampler(train)
    tail_ix, head_ix = sampler.indexes('cpu')
    tails, heads = {}, {}
    for h, t, r in zip(train.head_idx.tolist(), train.tail_idx.tolist(), train.relations.tolist()):
        tails.setdefault((h, r), set()).add(t)
        heads.setdefault((t, r), set()).add(h)
    assert index_as_dict(tail_ix) == tails and index_as_dict(head_ix) == heads
    assert sampler.indexes('cpu')[0] is tail_ix                             # built once per device
    # the child's inherited filter sets are the PARENT's: they hold facts the sampler's index must not
    parent = {k: set(v) for k, v in train.dict_of_tails.items()}
    assert sum(len(v) for v in parent.values()) == n > sum(len(v) for v in tails.values()) == train.n_facts
    assert any(t not in tails.get((h, r), ()) for h, t, r in zip(val.head_idx.tolist(), val.tail_idx.tolist(),
                                                                 val.relations.tolist()))
    assert sampler.exhaustible == 0                                          # no key lists 29 of 30 entities
    # filter_graphs: the known facts are those of the graphs named, laid end to end
    both = FilteredNegativeSampler(train, filter_graphs=(train, val))
    for h, t, r in zip(val.head_idx.tolist(), val.tail_idx.tolist(), val.relations.tolist()):
        tails.setdefault((h, r), set()).add(t)
    assert index_as_dict(both.indexes('cpu')[0]) == tails


def test_exhaustible_counts_the_keys_that_leave_fewer_than_two_entities_free():
    import torchkge_amd as tk
    from torchkge_amd.sampling import FilteredNegativeSampler
    n_ent = 6
    # (0, r0) knows 5 tails (one free), (1, r0) all 6, (2, r0) four (two free: not counted); on the head side tail 0 of
    # r0 has the heads {0, 1, 2}, no other tail more
    h = [0] * 5 + [1] * 6 + [2] * 4
    t = list(range(5)) + list(range(6)) + list(range(4))
    kg = tk.KnowledgeGraph(kg={'heads': torch.tensor(h), 'tails': torch.tensor(t), 'relations': torch.zeros(len(h), dtype=torch.int64)},
                           ent2ix={i: i for i in range(n_ent)}, rel2ix={0: 0})
    assert FilteredNegativeSampler(kg).exhaustible == 2


def test_parameter_lists_and_where_the_class_is_served():
    import torchkge_amd as tk
    from torchkge_amd import sampling
    from torchkge_amd.sampling import FilteredNegativeSampler, NegativeSampler, BernoulliNegativeSampler
    sig = inspect.signature(FilteredNegativeSampler.__init__)
    assert list(sig.parameters) == ['self', 'kg', 'kg_val', 'kg_test', 'n_neg', 'bernoulli', 'filter_graphs']
    assert [sig.parameters[k].default for k in ('kg_val', 'kg_test', 'n_neg', 'bernoulli', 'filter_graphs')] == [None, None, 1, True, None]
    for k in ('bernoulli', 'filter_graphs'):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters['n_neg'].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    csig = inspect.signature(FilteredNegativeSampler.corrupt_batch)
    assert list(csig.parameters) == ['self', 'heads', 'tails', 'relations', 'n_neg'] and csig.parameters['n_neg'].default is None
    assert csig == inspect.signature(BernoulliNegativeSampler.corrupt_batch)
    assert FilteredNegativeSampler.corrupt_kg is NegativeSampler.corrupt_kg             # inherited unchanged
    # one of the package's own samplers for Trainer; served on first access, not part of the package's dir()
    assert FilteredNegativeSampler.__module__ == BernoulliNegativeSampler.__module__ == sampling.__name__
    assert 'FilteredNegativeSampler' not in dir(tk) and tk.FilteredNegativeSampler is FilteredNegativeSampler
