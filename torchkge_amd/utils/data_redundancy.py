# -*- coding: utf-8 -*-
"""Data-redundancy analytics of Akrami et al. (`Realistic Re-evaluation of Knowledge Graph Completion Methods: An
Experimental Study <https://arxiv.org/pdf/2003.08001.pdf>`_, SIGMOD'20) on the HIP engine: the names, signatures and
return types of the reference's ``torchkge.utils.data_redundancy``.

The reference builds one Python set of (head, tail) pairs per relation and intersects them for every pair of relations.
Here one pass over sorted 64-bit keys (include/kge_hip_redundancy.h) gives two integer
matrices,

    same[r1][r2] = len(T[r1] & T[r2])          rev[r1][r2] = len(T[r1] & T_inv[r2])

and every function below reads them.  Every result is an integer or a comparison of two integers (the ratios are IEEE
double divisions of two integers, which is what Python's ``/`` computes), so the lists equal the reference's exactly.

The id tensors of the graphs may live on the CPU or on a GPU; they are moved to the current device.  Without a GPU the
functions raise RuntimeError: there is no CPU fallback.

Deliberate deviations from the reference:

* every relation of ``range(kg_tr.n_rel)`` is compared; the reference compares ``range(1345)`` (FB15k's count,
  hard-coded), raising KeyError on a smaller graph and ignoring the relations past 1345 of a larger one;
* a relation without facts never qualifies; the reference raises ZeroDivisionError;
* ``reverses`` filters the reverse list exactly as the reference's ``(r1, r2) not in reverses`` does;
* with ``counts=True`` the printed lines are the reference's, with the percentage multiplied by 100 on the "duplicate"
  lines too, where the reference forgot the factor;
* no ``tqdm`` progress bars.

``relation_overlaps`` is this engine's own addition: the matrices themselves, for trying several thresholds without
recounting."""
import torch

from .. import _hip_redundancy as _hr

__all__ = ['concat_kgs', 'get_pairs', 'count_triplets', 'duplicates', 'cartesian_product_relations', 'relation_overlaps']

_FIRST_CAP = 1 << 16        # pairs per list fetched by the one host read of duplicates(); more than that: a second pass


def concat_kgs(kg_tr, kg_val, kg_te):
    h = torch.cat((kg_tr.head_idx, kg_val.head_idx, kg_te.head_idx))
    t = torch.cat((kg_tr.tail_idx, kg_val.tail_idx, kg_te.tail_idx))
    r = torch.cat((kg_tr.relations, kg_val.relations, kg_te.relations))
    return h, t, r


def get_pairs(kg, r, type='ht'):
    """The set of (head, tail) pairs -- ``type='th'``: (tail, head) -- of relation ``r`` in ``kg``.  A plain host
    function, as in the reference; the functions of this module do not call it."""
    mask = (kg.relations == r)
    hs, ts = kg.head_idx[mask].tolist(), kg.tail_idx[mask].tolist()
    if type == 'ht':
        return set(zip(hs, ts))
    assert type == 'th'
    return set(zip(ts, hs))


def _check_ids(h, t, r, n_ent, n_rel):
    """ValueError for an id outside [0, n_ent) / [0, n_rel): the kernels index with them unchecked.  The check runs where
    the tensors live (on the host for CPU tensors; tensors already on a GPU pay one scalar read here)."""
    if h.shape[0] != t.shape[0] or h.shape[0] != r.shape[0]:
        raise ValueError('torchkge_amd: heads, tails and relations differ in length (%d, %d, %d)' % (h.shape[0], t.shape[0], r.shape[0]))
    if h.shape[0] == 0:
        return
    h_lo, t_lo, h_hi, t_hi, r_lo, r_hi = torch.stack([x.long() for x in (h.min(), t.min(), h.max(), t.max(), r.min(), r.max())]).tolist()
    e_lo, e_hi = min(h_lo, t_lo), max(h_hi, t_hi)
    if e_lo < 0 or e_hi >= n_ent:
        raise ValueError('torchkge_amd: entity ids span [%d, %d], outside [0, %d)' % (e_lo, e_hi, n_ent))
    if r_lo < 0 or r_hi >= n_rel:
        raise ValueError('torchkge_amd: relation ids span [%d, %d], outside [0, %d)' % (r_lo, r_hi, n_rel))


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('torchkge_amd runs only on MI355X (HIP) devices; torchkge_amd.utils.data_redundancy found none. '
                           'There is no CPU fallback.')
    return torch.device('cuda', torch.cuda.current_device())


def _facts(h, t, r, n_ent, n_rel):
    """Checked (h, t, r) as int64 tensors on the current device."""
    _check_ids(h, t, r, n_ent, n_rel)
    dev = _device()
    return tuple(x.to(device=dev, dtype=torch.int64) for x in (h, t, r))


def relation_overlaps(kg_tr, kg_val, kg_te, rev=True, max_bytes=1 << 30):
    """The counts behind ``duplicates`` as device tensors ``(lengths, same, rev)``, over the union of the three graphs:

    * ``lengths`` int64 (n_rel): facts per relation, repeats included (the reference's ``mask.sum()``);
    * ``same`` int32 (n_rel, n_rel): ``same[r1][r2] = len(T[r1] & T[r2])``; the diagonal is ``len(T[r])``;
    * ``rev`` int32 (n_rel, n_rel): ``rev[r1][r2] = len(T[r1] & T_inv[r2])``, symmetric; None when ``rev`` is false.

    ValueError when the matrices would take more than ``max_bytes`` bytes, or when an id lies outside the graph's
    ``n_ent`` / ``n_rel``; both before any device work."""
    n_ent, n_rel = kg_tr.n_ent, kg_tr.n_rel
    need = (2 if rev else 1) * n_rel * n_rel * 4
    if need > max_bytes:
        raise ValueError('torchkge_amd: the relation-overlap matrices of %d relations take %d bytes, more than max_bytes = %d'
                         % (n_rel, need, max_bytes))
    h, t, r = _facts(*concat_kgs(kg_tr, kg_val, kg_te), n_ent, n_rel)
    lengths = _hr.relation_stats(h, t, r, n_ent, n_rel)[0]
    same, rv = _hr.relation_overlap((h, t, r), None, n_ent, n_rel, want_rev=rev)
    return lengths, same, rv


def _select_both(lengths, same, rev, theta1, theta2):
    """The two selected pair lists as int lists of lists, from ONE host read (a second pass only when a list is longer
    than _FIRST_CAP pairs)."""
    n_rel = same.shape[0]
    full = n_rel * (n_rel - 1) // 2
    cap = max(min(full, _FIRST_CAP), 1)
    while True:
        # one buffer: [n_dup, n_rev] as two int64, then the two (cap, 2) int32 lists
        buf = torch.empty(4 + 4 * cap, dtype=torch.int32, device=same.device)
        n_out = buf[:4].view(torch.int64)
        lists = buf[4:].view(2, cap, 2)
        _hr.overlap_select(same, lengths, theta1, theta2, lists[0], n_out[0:1])
        _hr.overlap_select(rev, lengths, theta1, theta2, lists[1], n_out[1:2])
        host = buf.cpu()
        n_dup, n_rev = host[:4].view(torch.int64).tolist()
        if max(n_dup, n_rev) <= cap:
            pairs = host[4:].view(2, cap, 2)
            return pairs[0, :n_dup].tolist(), pairs[1, :n_rev].tolist()
        cap = full


def duplicates(kg_tr, kg_val, kg_te, theta1=0.8, theta2=0.8, verbose=False, counts=False, reverses=None):
    """Return the duplicate and reverse duplicate relations as explained in the paper by Akrami et al.

    Parameters
    ----------
    kg_tr, kg_val, kg_te: torchkge_amd.data_structures.KnowledgeGraph
        Train, validation and test sets.
    theta1, theta2: float
        The two thresholds (see paper): a pair (r1, r2), r1 < r2, is kept when
        ``len(T[r1] & T[r2]) / lengths[r1] > theta1 and len(T[r1] & T[r2]) / lengths[r2] > theta2``.
    verbose: bool
    counts: bool
        Should the triplets involving (reverse) duplicate relations be counted in all sets (printed).
    reverses: list
        List of known reverse relations: pairs that are left out of the reverse list.

    Returns
    -------
    duplicates, rev_duplicates: two lists of (int, int) tuples, in the order of ``itertools.combinations``.

    See the module docstring for the deviations from the reference (every relation of ``range(kg_tr.n_rel)``, empty
    relations, the printed percentages, no progress bars).  One host read fetches both lists."""
    if verbose:
        print('Computing Ts')
    if reverses is None:
        reverses = []
    lengths, same, rev = relation_overlaps(kg_tr, kg_val, kg_te)
    if verbose:
        print('Finding duplicate relations')
    dup, rdup = _select_both(lengths, same, rev, theta1, theta2)
    dup = [(a, b) for a, b in dup]
    rdup = [(a, b) for a, b in rdup if (a, b) not in reverses]
    if verbose:
        print('Duplicate relations: {}'.format(len(dup)))
        print('Reverse duplicate relations: {}\n'.format(len(rdup)))
    if counts:
        for kg1, kg2, what, where in ((kg_tr, kg_tr, 'train', 'train'), (kg_tr, kg_te, 'test', 'train'),
                                      (kg_te, kg_te, 'test', 'test')):
            n_dup, n_rev = count_triplets(kg1, kg2, dup, rdup)
            print('{} {} triplets have duplicate in {} set '
                  '({}%)'.format(n_dup, what, where, int(n_dup / len(kg2) * 100)))
            print('{} {} triplets have reverse duplicate in {} set '
                  '({}%)\n'.format(n_rev, what, where, int(n_rev / len(kg2) * 100)))
    return dup, rdup


def count_triplets(kg1, kg2, duplicates, rev_duplicates):
    """
    Parameters
    ----------
    kg1, kg2: torchkge_amd.data_structures.KnowledgeGraph
    duplicates, rev_duplicates: list
        Lists returned by torchkge_amd.utils.data_redundancy.duplicates.

    Returns
    -------
    n_duplicates: int
        Number of triplets in kg2 that have their duplicate triplet in kg1.
    n_rev_duplicates: int
        Number of triplets in kg2 that have their reverse duplicate triplet in kg1.

    One rectangular count (A = kg2, B = kg1) and one host read of the two sums:
    ``sum(same[r1][r2] + same[r2][r1])`` over ``duplicates``, the same of ``rev`` over ``rev_duplicates``."""
    n_ent, n_rel = kg1.n_ent, kg1.n_rel
    for lst in (duplicates, rev_duplicates):
        for r1, r2 in lst:
            if not (0 <= r1 < n_rel and 0 <= r2 < n_rel):
                raise ValueError('torchkge_amd: relation pair (%d, %d) outside [0, %d)' % (r1, r2, n_rel))
    a = _facts(kg2.head_idx, kg2.tail_idx, kg2.relations, n_ent, n_rel)
    b = None if kg1 is kg2 else _facts(kg1.head_idx, kg1.tail_idx, kg1.relations, n_ent, n_rel)
    same, rev = _hr.relation_overlap(a, b, n_ent, n_rel, want_rev=True)
    sums = torch.zeros(2, dtype=torch.int64, device=same.device)
    for i, (mat, lst) in enumerate(((same, duplicates), (rev, rev_duplicates))):
        if len(lst):
            p = torch.tensor(list(lst), dtype=torch.int64).view(-1, 2).to(same.device)
            sums[i] = mat[p[:, 0], p[:, 1]].sum(dtype=torch.int64) + mat[p[:, 1], p[:, 0]].sum(dtype=torch.int64)
    n_dup, n_rev = sums.tolist()
    return n_dup, n_rev


def cartesian_product_relations(kg_tr, kg_val, kg_te, theta=0.8):
    """Return the cartesian product relations as explained in the paper by Akrami et al.: the relations r with
    ``lengths[r] / (len(S[r]) * len(O[r])) > theta``, S and O the distinct heads and tails of r over the three graphs.

    The three integer vectors come from the device in one read; the ratio is computed on the host in Python, as the
    reference computes it.  A relation without facts never qualifies (the reference raises ZeroDivisionError).

    Returns
    -------
    selected_relations: list of int"""
    n_ent, n_rel = kg_tr.n_ent, kg_tr.n_rel
    h, t, r = _facts(*concat_kgs(kg_tr, kg_val, kg_te), n_ent, n_rel)
    lengths, n_s, n_o = _hr.relation_stats(h, t, r, n_ent, n_rel).tolist()
    return [r_ for r_ in range(n_rel) if lengths[r_] > 0 and lengths[r_] / (n_s[r_] * n_o[r_]) > theta]
