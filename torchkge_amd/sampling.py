# -*- coding: utf-8 -*-
"""Negative samplers with the reference's interface (torchkge/sampling.py:16-592):
``NegativeSampler``, ``UniformNegativeSampler``, ``BernoulliNegativeSampler``
(``.bern_probs``, ``.corrupt_batch(heads, tails, relations, n_neg=None)``,
``.corrupt_kg(batch_size, use_cuda, which, on_device=False, n_neg=1)``), ``PositionalNegativeSampler``
(``.possible_heads / .possible_tails / .n_poss_heads / .n_poss_tails``),
``BernoulliRelationNegativeSampler`` (``.bern_probs``, ``.rel_share``; three
vectors out) and ``get_possible_heads_tails``.

The random draws are issued with the same torch RNG calls, in the same order
and with the same sizes as the reference (bernoulli, randint(k),
randint(B*n_neg - k)), so under the same seed and device the samples are the
reference's; the masked index-puts (the integer part) run in one HIP scatter
(kge_corrupt_scatter).  ``sync_free=True`` draws B*n_neg replacements for both
sides instead, removing the device->host sync of ``mask.sum().item()`` at the
price of a different (equally distributed) random stream.

The positional sampler keeps its two possibility indices as dense per-relation
CSRs on the device and corrupts a batch in one gather (kge_positional_corrupt):
no Python loop over the facts of the graph or the elements of a batch.

The relation-corrupting sampler's three masked index-puts are one HIP entry
point as well (kge_relation_corrupt, include/kge_hip_relation.h): two dependent
prefix counts and one scatter.

``FilteredNegativeSampler`` (the engine's own) draws every replacement exactly
over the entities that are not known answers of the fact's key, from two
device-resident FilterIndexes and one kernel (kge_filtered_corrupt,
include/kge_hip_filtered.h): no rejection loop, no host read.
"""
from collections import defaultdict

import torch
from torch import bernoulli, cat, ones, rand, randint, tensor

from . import _hip, _hip_filtered, _hip_relation, _hip_triplet
from .exceptions import NotYetImplementedError
from .filter_index import FilterIndex, KEY2_SPAN
from .utils.data import DataLoader
from .utils.operations import get_bernoulli_probs


def _check_block(sampler, neg, facts, n_neg):
    """A corrupt_batch that ignores ``n_neg`` (one negative per fact whatever it is asked) cannot serve corrupt_kg(n_neg > 1)."""
    if n_neg != 1 and neg.shape[0] != n_neg * facts.shape[0]:
        raise ValueError('%s.corrupt_batch returned %d negatives for %d facts with n_neg = %d: this sampler draws one '
                         'negative per fact' % (type(sampler).__name__, neg.shape[0], facts.shape[0], n_neg))


class NegativeSampler:
    """Interface (sampling.py:16-138)."""

    def __init__(self, kg, kg_val=None, kg_test=None, n_neg=1):
        self.kg = kg
        self.n_ent = kg.n_ent
        self.n_facts = kg.n_facts
        self.kg_val = kg_val
        self.kg_test = kg_test
        self.n_neg = n_neg
        self.n_facts_val = 0 if kg_val is None else kg_val.n_facts
        self.n_facts_test = 0 if kg_test is None else kg_test.n_facts
        self.sync_free = False
        self._device_graphs = {}        # id(graph) -> its three vectors on the GPU (corrupt_kg(on_device=True))

    def _device_graph(self, kg):
        """(heads, tails, relations) of ``kg`` on the GPU, uploaded once per sampler."""
        hit = self._device_graphs.get(id(kg))
        if hit is None:
            hit = self._device_graphs[id(kg)] = (kg.head_idx.cuda(), kg.tail_idx.cuda(), kg.relations.cuda())
        return hit

    def corrupt_batch(self, heads, tails, relations, n_neg):
        raise NotYetImplementedError('NegativeSampler is just an interface, please consider using '
                                     'a child class where this is implemented.')

    def corrupt_kg(self, batch_size, use_cuda, which='main', on_device=False, *, n_neg=1):
        """Corrupt a whole graph batch by batch with n_neg=1 by default (sampling.py:76-138): the reference's driver, host tensors
        out.  ``on_device=True`` takes the graph's vectors to the GPU once, corrupts slices of them and returns the two
        negative vectors as device tensors: nothing goes through the host (what TrainDataLoader with use_cuda='all' and
        TripletClassificationEvaluator use).

        ``n_neg`` (the engine's own, keyword only): negatives per fact.  The output is the batches laid end to end, the
        block of a batch of B_b facts being its ``n_neg * B_b`` positions in tile order (negative k of the batch's fact i at
        ``k * B_b + i``, as ``corrupt_batch`` returns them).  1 is the reference's output and random stream."""
        assert which in ['main', 'train', 'test', 'val']
        if which == 'val':
            assert self.n_facts_val > 0
        if which == 'test':
            assert self.n_facts_test > 0
        kg = self.kg_val if which == 'val' else (self.kg_test if which == 'test' else self.kg)
        corr_heads, corr_tails = [], []
        if on_device:
            assert kg is not None and kg.n_facts > 0
            h, t, r = self._device_graph(kg)
            for lo in range(0, h.shape[0], batch_size):
                sl = slice(lo, lo + batch_size)
                neg_heads, neg_tails = self.corrupt_batch(h[sl], t[sl], r[sl], n_neg=n_neg)
                _check_block(self, neg_heads, h[sl], n_neg)
                corr_heads.append(neg_heads)
                corr_tails.append(neg_tails)
            return cat(corr_heads).long(), cat(corr_tails).long()
        tmp_cuda = 'batch' if use_cuda else None
        dataloader = DataLoader(kg, batch_size=batch_size, use_cuda=tmp_cuda)
        for batch in dataloader:
            neg_heads, neg_tails = self.corrupt_batch(batch[0], batch[1], batch[2], n_neg=n_neg)
            _check_block(self, neg_heads, batch[0], n_neg)
            corr_heads.append(neg_heads)
            corr_tails.append(neg_tails)
        if use_cuda:
            return cat(corr_heads).long().cpu(), cat(corr_tails).long().cpu()
        return cat(corr_heads).long(), cat(corr_tails).long()

    # shared by the Uniform and Bernoulli samplers
    def _corrupt(self, heads, tails, probs, n_neg):
        device = heads.device
        assert device == tails.device
        _hip.require_cuda(heads, tails)
        batch_size = heads.shape[0]
        n = batch_size * n_neg
        mask = bernoulli(probs)                                  # RNG draw #1
        if self.sync_free:
            draws_h = randint(1, self.n_ent, (n,), device=device)
            draws_t = randint(1, self.n_ent, (n,), device=device)
            # position j consumes draw #(ones before j); any fixed assignment is
            # equally distributed, the scatter kernel keeps the prefix-sum rule
        else:
            n_h_cor = int(mask.sum().item())                     # the reference's sync (:319)
            draws_h = randint(1, self.n_ent, (n_h_cor,), device=device)       # draw #2
            draws_t = randint(1, self.n_ent, (n - n_h_cor,), device=device)   # draw #3
        return _hip.corrupt_scatter(heads, tails, mask.to(torch.uint8), draws_h, draws_t, n_neg)


class UniformNegativeSampler(NegativeSampler):
    """Head or tail replaced with probability 1/2 (sampling.py:141-223)."""

    def __init__(self, kg, kg_val=None, kg_test=None, n_neg=1):
        super().__init__(kg, kg_val, kg_test, n_neg)

    def corrupt_batch(self, heads, tails, relations=None, n_neg=None):
        if n_neg is None:
            n_neg = self.n_neg
        probs = ones(size=(heads.shape[0] * n_neg,), device=heads.device) / 2
        return self._corrupt(heads, tails, probs, n_neg)


class BernoulliNegativeSampler(NegativeSampler):
    """Head replaced with probability tph/(tph+hpt) of the relation
    (Wang et al. 2014; sampling.py:226-327)."""

    def __init__(self, kg, kg_val=None, kg_test=None, n_neg=1):
        super().__init__(kg, kg_val, kg_test, n_neg)
        self.bern_probs = self.evaluate_probabilities()

    def evaluate_probabilities(self):
        """fp32 (n_rel) vector, 0.5 for relations absent from the graph
        (sampling.py:263-276)."""
        bern_probs = get_bernoulli_probs(self.kg)
        tmp = []
        for i in range(self.kg.n_rel):
            tmp.append(bern_probs[i] if i in bern_probs.keys() else 0.5)
        return tensor(tmp).float()

    def corrupt_batch(self, heads, tails, relations, n_neg=None):
        if n_neg is None:
            n_neg = self.n_neg
        self.bern_probs = self.bern_probs.to(heads.device)
        return self._corrupt(heads, tails, self.bern_probs[relations].repeat(n_neg), n_neg)


class FilteredNegativeSampler(NegativeSampler):
    """Head or tail (Bernoulli choice of Wang et al. 2014, or 1/2 with ``bernoulli=False``) replaced by an entity drawn
    EXACTLY and uniformly over the entities that are not known answers: a replaced tail of (h, r, t) is neither a known
    tail of (h, r) nor t itself, a replaced head neither a known head of (t, r) nor h itself.  No negative is a known
    fact and none equals its own fact -- also for a fact that is not among the known ones.  The engine's own: the
    reference has no filtered sampler.

    The known facts are those of ``filter_graphs`` (default ``(kg,)``), kept as two ``FilterIndex``es -- (h, r) -> tails
    and (t, r) -> heads -- built from the graphs' OWN triples once per device on first use.  ``kg.filter_index`` is NOT
    used: a child of ``split_kg`` shares its parent's lazy dictionaries, so that index holds the validation and test
    facts as well, and a sampler that avoided them would leak the evaluation sets into training.

    Random calls of ``corrupt_batch``, on the batch's device (n = B * n_neg): ``bernoulli(bern_probs[relations]
    .repeat(n_neg))`` (``bernoulli=False``: of a vector of 1/2) and ``randint(0, 2**62, (n,))``; then two lookups of the
    B keys and one kge_filtered_corrupt (include/kge_hip_filtered.h), which reduces a draw modulo the number c of free
    entities of its position and picks the draw-th of them in ascending order.  Both sizes depend on (B, n_neg) alone:
    nothing is ever read back, ``sync_free`` is accepted and changes nothing.  The modulo bias is below n_ent / 2**62.

    ``exhaustible``: the number of keys whose list leaves fewer than two entities free (read once, when the index is
    built).  Only a position of such a key can find no free entity; it then keeps its fact unchanged.  While
    ``exhaustible`` is 0 the kernel writes no flags; otherwise ``last_exhausted`` holds the uint8 flags of the last batch
    (tile order, 1 = the fact came back unchanged)."""

    def __init__(self, kg, kg_val=None, kg_test=None, n_neg=1, *, bernoulli=True, filter_graphs=None):
        super().__init__(kg, kg_val, kg_test, n_neg)
        self.n_rel = kg.n_rel
        self.bernoulli = bool(bernoulli)
        self.bern_probs = self.evaluate_probabilities() if self.bernoulli else None
        self.filter_graphs = (kg,) if filter_graphs is None else tuple(filter_graphs)
        self._index = {}            # device -> ((h, r) -> tails, (t, r) -> heads)
        self._exhaustible = None
        self.last_exhausted = None

    evaluate_probabilities = BernoulliNegativeSampler.evaluate_probabilities

    def indexes(self, device=None):
        """``(tail index, head index)`` of the known facts on ``device`` (default: where the graph's vectors are), built
        on first use -- on the GPU by the library's own index builder."""
        device = self.kg.head_idx.device if device is None else torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        hit = self._index.get(device)
        if hit is None:
            h, t, r = _graph_triples(*self.filter_graphs)
            hit = self._index[device] = (FilterIndex.from_triples_torch(h, r, t, device, self.n_ent, self.n_rel, self.n_ent),
                                         FilterIndex.from_triples_torch(t, r, h, device, self.n_ent, self.n_rel, self.n_ent))
            if self._exhaustible is None:       # the one host read, at index build
                self._exhaustible = sum(int(((ix.offsets[1:] - ix.offsets[:-1]) > self.n_ent - 2).sum().item()) for ix in hit)
        return hit

    @property
    def exhaustible(self):
        if self._exhaustible is None:
            self.indexes()
        return self._exhaustible

    def corrupt_batch(self, heads, tails, relations, n_neg=None):
        if n_neg is None:
            n_neg = self.n_neg
        device = heads.device
        assert device == tails.device
        _hip.require_cuda(heads, tails, relations)
        n = heads.shape[0] * n_neg
        tail_ix, head_ix = self.indexes(device)
        tail_lo, tail_hi = tail_ix.lookup(heads, relations)
        head_lo, head_hi = head_ix.lookup(tails, relations)
        if self.bernoulli:
            self.bern_probs = self.bern_probs.to(device)
            probs = self.bern_probs[relations].repeat(n_neg)
        else:
            probs = ones(size=(n,), device=device) / 2
        mask = bernoulli(probs)                                         # RNG draw #1
        draws = randint(0, 2 ** 62, (n,), device=device)                # draw #2
        neg_h, neg_t, self.last_exhausted = _hip_filtered.filtered_corrupt(
            heads, tails, mask.to(torch.uint8), draws, tail_lo, tail_hi, tail_ix.targets, head_lo, head_hi,
            head_ix.targets, self.n_ent, n_neg, want_exhausted=self._exhaustible > 0)
        return neg_h, neg_t

    def known(self, heads, tails, relations):
        """bool mask: which of the triples ``(heads, relations, tails)`` are facts of ``filter_graphs`` (one
        kge_triples_known against the tail index).  Works for the output of any sampler: with ``relations`` repeated
        n_neg times it counts the false negatives of a batch."""
        _hip.require_cuda(heads, tails, relations)
        tail_ix, _ = self.indexes(heads.device)
        return _hip_filtered.triples_known(tail_ix.keys, tail_ix.offsets, tail_ix.targets, KEY2_SPAN, heads, relations,
                                           tails).bool()


class _PossibilityIndex(object):
    """Dense per-relation CSR of one side: the distinct entities seen at that place of relation r are
    ``values[offsets[r]:offsets[r + 1]]`` (int32, ascending); ``offsets`` is int64 (n_rel + 1)."""

    def __init__(self, relations, entities, n_rel, n_ent, device):
        # sort / unique by the engine's index builder (key1 = relation, key2 = 0, value = entity): rocPRIM on the GPU,
        # ATen elsewhere; its sorted-key CSR lists only the relations that occur, the counts scatter makes it dense
        zeros = torch.zeros_like(relations)
        idx = FilterIndex.from_triples_torch(relations, zeros, entities, device, n_rel, 1, n_ent)
        counts = torch.zeros(n_rel, dtype=torch.int64, device=idx.offsets.device)
        if idx.n_keys:
            counts[idx.keys // KEY2_SPAN] = idx.offsets[1:] - idx.offsets[:-1]
        self.offsets = torch.zeros(n_rel + 1, dtype=torch.int64, device=counts.device)
        self.offsets[1:] = torch.cumsum(counts, 0)
        self.values = idx.targets       # (one zero when the graph is empty: a valid pointer, never inside a segment)
        self.counts = counts

    def to(self, device):
        out = object.__new__(_PossibilityIndex)
        out.offsets, out.values, out.counts = self.offsets.to(device), self.values.to(device), self.counts.to(device)
        return out

    def lists(self):
        """{r: ascending list of entities}, every relation a key."""
        off, val = self.offsets.cpu().tolist(), self.values.cpu().numpy()
        return {r: val[off[r]:off[r + 1]].tolist() for r in range(len(off) - 1)}


def _graph_triples(*kgs):
    """(heads, tails, relations) of the graphs laid end to end."""
    kgs = [g for g in kgs if g is not None and g.n_facts > 0]
    if not kgs:
        e = torch.zeros(0, dtype=torch.int64)
        return e, e, e
    dev = kgs[0].head_idx.device
    return tuple(cat([getattr(g, nm).to(dev) for g in kgs]) for nm in ('head_idx', 'tail_idx', 'relations'))


def get_possible_heads_tails(kg, possible_heads=None, possible_tails=None):
    """{relation: set of entities seen as its head}, {relation: set seen as its tail} of ``kg``, merged into the two
    dicts of an earlier call when they are given (sampling.py:556-592).  Only relations that occur are keys.  One
    sort / unique over the facts instead of three ``.item()`` calls per fact."""
    out = []
    for given, ents in ((possible_heads, kg.head_idx), (possible_tails, kg.tail_idx)):
        if given is None:
            d = defaultdict(set)
        else:
            assert type(given) == dict
            d = defaultdict(set, given)
        if kg.n_facts > 0:
            idx = _PossibilityIndex(kg.relations, ents, kg.n_rel, kg.n_ent, kg.relations.device)
            for r, vals in idx.lists().items():
                if vals:
                    d[r].update(vals)
        out.append(dict(d))
    return out[0], out[1]


class PositionalNegativeSampler(BernoulliNegativeSampler):
    """Head or tail (Bernoulli choice of Wang et al. 2014) replaced by an entity that occupies the same place in
    another fact of the same relation (Socher et al. 2013; sampling.py:330-504).  The possibilities come from ``kg``
    and ``kg_val``, never from ``kg_test``; a relation without any gets a uniform entity of [0, n_ent).

    ``possible_heads`` / ``possible_tails``: {relation: list}, every relation of range(n_rel) a key, built on first
    access; ``n_poss_heads`` / ``n_poss_tails``: int64 (n_rel).

    Difference from the reference: within a relation the entities are in ASCENDING id order, where the reference has
    ``list(set)`` order (an artefact of CPython's hash table).  The draw is uniform over the same set either way, but
    the same seed picks a different member.

    Random calls, on the batch's device and in the reference's order: ``bernoulli(bern_probs[relations])``, one host
    read of the number k of heads to replace, ``rand((k,))``, ``rand((B - k,))``; then ``randint(0, n_ent, (k,))`` and
    ``randint(0, n_ent, (B - k,))`` only when the sampler holds a relation without possibilities.  With
    ``sync_free = True`` all four arrays are B long and nothing is read back: the same kernel, a different but equally
    distributed stream."""

    def __init__(self, kg, kg_val=None, kg_test=None):
        super().__init__(kg, kg_val, kg_test, 1)
        h, t, r = _graph_triples(kg, kg_val if self.n_facts_val > 0 else None)
        self.n_rel = kg.n_rel
        self._index = {}        # device -> (heads index, tails index)
        self._index[h.device] = (_PossibilityIndex(r, h, self.n_rel, self.n_ent, h.device),
                                 _PossibilityIndex(r, t, self.n_rel, self.n_ent, h.device))
        ih, it = self._index[h.device]
        self.n_poss_heads, self.n_poss_tails = ih.counts.cpu(), it.counts.cpu()
        # (head and tail of a relation are empty together: both come from the same facts)
        self._has_empty = bool((self.n_poss_heads == 0).any()) if self.n_rel > 0 else False
        self._lists = None

    def _indices(self, device):
        if device not in self._index:
            ih, it = next(iter(self._index.values()))
            self._index[device] = (ih.to(device), it.to(device))
        return self._index[device]

    def _possible(self):
        if self._lists is None:
            ih, it = next(iter(self._index.values()))
            self._lists = (ih.lists(), it.lists())
        return self._lists

    @property
    def possible_heads(self):
        return self._possible()[0]

    @property
    def possible_tails(self):
        return self._possible()[1]

    def find_possibilities(self):
        """(possible_heads, possible_tails, n_poss_heads, n_poss_tails), as the reference returns them."""
        return self.possible_heads, self.possible_tails, self.n_poss_heads, self.n_poss_tails

    def corrupt_batch(self, heads, tails, relations, n_neg=None):
        """One negative per fact (``n_neg`` is part of the samplers' interface only, as in the reference)."""
        device = heads.device
        assert device == tails.device
        _hip.require_cuda(heads, tails, relations)
        B = heads.shape[0]
        self.bern_probs = self.bern_probs.to(device)
        mask = bernoulli(self.bern_probs[relations])                # RNG draw #1
        if self.sync_free:
            k_h = k_t = B
        else:
            k_h = int(mask.sum().item())                            # the reference's sync (:463)
            k_t = B - k_h
        u_h = rand((k_h,), device=device)                           # draw #2
        u_t = rand((k_t,), device=device)                           # draw #3
        fb_h = fb_t = None
        if self._has_empty:
            fb_h = randint(0, self.n_ent, (k_h,), device=device)
            fb_t = randint(0, self.n_ent, (k_t,), device=device)
        ih, it = self._indices(device)
        return _hip_triplet.positional_corrupt(heads, tails, relations, mask.to(torch.uint8), u_h, u_t, fb_h, fb_t,
                                               ih.offsets, ih.values, it.offsets, it.values, self.n_rel)


class BernoulliRelationNegativeSampler(NegativeSampler):
    """Corrupts either the relation of a fact or, with the Bernoulli choice of Wang et al. 2014, its head or its tail
    (sampling.py:507-553).  ``corrupt_batch`` returns ``(neg_heads, neg_tails, neg_rels)``, int64 on the batch's device.

    The reference's quirks are kept:
      * ``rel_share`` is the probability that an ENTITY is corrupted (the reference's own comment: "if 1 then entities
        are corrupted"), so the relation is corrupted with probability ``1 - rel_share``;
      * every draw is ``randint(1, .)``: neither entity 0 nor relation 0 is ever drawn;
      * the drawn relation may equal the true one;
      * a graph of one relation raises torch's own error from ``randint(1, 1)``.

    Two deliberate differences:
      * ``n_neg`` is honoured: the batch is repeated ``n_neg`` times as in ``BernoulliNegativeSampler`` and 3 x
        (B * n_neg) ids come back (the reference ignores it and returns B negatives);
      * ``corrupt_kg`` returns three vectors (the reference inherits a ``corrupt_kg`` that unpacks two and raises);
        ``on_device=True`` keeps the graph's vectors and the negatives on the GPU, as in ``PositionalNegativeSampler``.

    Random calls, on the batch's device, in the reference's order and with its sizes (n = B * n_neg):
    ``bernoulli(rel_share * ones(n))``, one host read of its sum k, ``randint(1, n_rel, (n - k,))``,
    ``bernoulli(bern_probs[relations.repeat(n_neg)[mask == 1]])``, one host read of its sum q,
    ``randint(1, n_ent, (q,))``, ``randint(1, n_ent, (k - q,))``; then one kge_relation_corrupt.  With
    ``sync_free = True`` all five arrays are n long and nothing is read back: the head mask is drawn for every position
    from ``bern_probs[relations.repeat(n_neg)]`` and the entity positions' entries are moved to the front on the device
    (the kernel consumes it compactly), so every position still uses the probability of its own relation.  The same
    kernel, a different but equally distributed stream."""

    def __init__(self, kg, kg_val=None, kg_test=None, n_neg=1, rel_share=.33):
        super().__init__(kg, kg_val, kg_test, n_neg)
        self.n_rel = kg.n_rel
        self.bern_probs = self.evaluate_probabilities()
        self.rel_share = rel_share

    evaluate_probabilities = BernoulliNegativeSampler.evaluate_probabilities

    def corrupt_batch(self, heads, tails, relations, n_neg=None):
        if n_neg is None:
            n_neg = self.n_neg
        device = heads.device
        assert device == tails.device
        _hip.require_cuda(heads, tails, relations)
        n = heads.shape[0] * n_neg
        self.bern_probs = self.bern_probs.to(device)
        rels_rep = relations.repeat(n_neg)
        mask_ent = bernoulli(self.rel_share * ones(n, device=device))            # RNG draw #1: 1 = an entity is corrupted
        if self.sync_free:
            draws_r = randint(1, self.n_rel, (n,), device=device)
            side = bernoulli(self.bern_probs[rels_rep])         # the head / tail choice of position j, were it an entity's
            # the kernel reads the choice of the p-th ENTITY position at mask_head[p]: move every position's own choice
            # there (the other positions' behind them, a permutation) -- a position keeps the probability of ITS relation
            ones_upto = torch.cumsum(mask_ent, 0).long()
            at = torch.arange(n, device=device)
            slot = torch.where(mask_ent != 0, ones_upto - 1, ones_upto[-1:] + at - ones_upto) if n else at
            mask_head = torch.empty_like(side).scatter_(0, slot, side)
            draws_h = randint(1, self.n_ent, (n,), device=device)
            draws_t = randint(1, self.n_ent, (n,), device=device)
            # (the draws are i.i.d.: position j consumes the entries its two prefix counts name, any fixed assignment is
            # equally distributed)
        else:
            k = int(mask_ent.sum().item())                                       # the reference's sync (:538)
            draws_r = randint(1, self.n_rel, (n - k,), device=device)            # draw #2
            mask_head = bernoulli(self.bern_probs[rels_rep[mask_ent == 1]])      # draw #3
            q = int(mask_head.sum().item())                                      # the reference's sync (:548)
            draws_h = randint(1, self.n_ent, (q,), device=device)                # draw #4
            draws_t = randint(1, self.n_ent, (k - q,), device=device)            # draw #5
        return _hip_relation.relation_corrupt(heads, tails, relations, mask_ent.to(torch.uint8), mask_head.to(torch.uint8),
                                              draws_r, draws_h, draws_t, n_neg)

    def corrupt_kg(self, batch_size, use_cuda, which='main', on_device=False, *, n_neg=1):
        """(neg_heads, neg_tails, neg_rels) of a whole graph, batch by batch with n_neg = 1 by default: host tensors, or
        with ``on_device=True`` device tensors from vectors that never leave the GPU.  ``n_neg``: negatives per fact, every
        batch's block in tile order (NegativeSampler.corrupt_kg)."""
        assert which in ['main', 'train', 'test', 'val']
        if which == 'val':
            assert self.n_facts_val > 0
        if which == 'test':
            assert self.n_facts_test > 0
        kg = self.kg_val if which == 'val' else (self.kg_test if which == 'test' else self.kg)
        out = ([], [], [])
        if on_device:
            h, t, r = self._device_graph(kg)
            batches = ((h[lo:lo + batch_size], t[lo:lo + batch_size], r[lo:lo + batch_size])
                       for lo in range(0, h.shape[0], batch_size))
        else:
            batches = DataLoader(kg, batch_size=batch_size, use_cuda='batch' if use_cuda else None)
        for batch in batches:
            for lst, neg in zip(out, self.corrupt_batch(batch[0], batch[1], batch[2], n_neg=n_neg)):
                lst.append(neg)
        empty = torch.zeros(0, dtype=torch.int64)
        out = tuple(cat(lst).long() if lst else empty for lst in out)
        return out if on_device or not use_cuda else tuple(x.cpu() for x in out)
