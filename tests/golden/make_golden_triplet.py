# -*- coding: utf-8 -*-
"""Generate the triplet-classification golden fixture in this directory by RUNNING THE REAL
REFERENCE (torchkge v0.17.7 imported from /root/reference, CPU).  Run in the build
container only (the reference does not exist on the GPU box):

    python tests/golden/make_golden_triplet.py

Output (committed): tests/golden/ref_triplet.npz, written with fixed archive timestamps so that
a second run gives the same bytes.

Graph: make_golden.make_kg(0).  Validation = facts [0, 400) without relation 5, test = facts
[400, 700): relation 5 has no possibilities, so its positions take the reference's uniform fallback.

Sampler part.  The reference's PositionalNegativeSampler keeps each relation's possibilities in
``list(set)`` order; the engine keeps them ascending.  The fixture is produced by the unmodified
reference code on SORTED lists (``possible_*[r].sort()``: data, not code), and the random draws it
consumed are recorded by replaying the same torch RNG calls under the same seed:
bernoulli(bern_probs[r]), rand(k), rand(B - k), then one randint(0, n_ent, (1,)) per position of an
empty relation, heads first.  Each single fallback draw is stored at the index its position
consumes (fb_h[p] for the p-th head position); the unused entries are -1.  Asserted here:
  * the replay against the UNSORTED lists reproduces the untouched reference call exactly
    (so the order of draws is understood), and
  * the replay against the sorted lists reproduces the recorded outputs exactly.

Evaluator part, for the six model kinds of tests/test_gpu_parity.py::CASES (make_golden.build_model
with make_golden's perturbation; the tables must equal the ones committed in ref_<kind>.npz, they
are not stored twice): the reference's thresholds, the scores of its validation negatives, its test
positive / negative scores, its number of correct decisions and the number of decisions whose
score lies within NEAR = 2e-5 of its threshold -- twice the project's score tolerance 1e-5: an
engine score and an engine threshold each lie within 1e-5 of the reference's, so only such
decisions can come out differently.  Asserted: at most 2 % of the 600 decisions per model.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchkge  # noqa: E402
from torchkge.data_structures import KnowledgeGraph  # noqa: E402
from torchkge.evaluation import TripletClassificationEvaluator  # noqa: E402
from torchkge.sampling import PositionalNegativeSampler  # noqa: E402
from make_golden import make_kg, build_model, tables_of, N_ENT, N_REL  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
assert torchkge.__version__ == '0.17.7'
B_SIZE = 64
EMPTY_REL = 5
NEAR = 2e-5
SEEDS = {'main': 11, 'test': 12}
CASES = [('transe', 2), ('transe', 1), ('transh', 2), ('transd', 2), ('distmult', 2), ('complex', 2)]


def split(kg, lo, hi, drop_rel=None):
    h, t, r = kg.head_idx[lo:hi], kg.tail_idx[lo:hi], kg.relations[lo:hi]
    if drop_rel is not None:
        keep = r != drop_rel
        h, t, r = h[keep], t[keep], r[keep]
    return KnowledgeGraph(kg={'heads': h.clone(), 'tails': t.clone(), 'relations': r.clone()}, ent2ix=kg.ent2ix,
                          rel2ix=kg.rel2ix)


def replay(samp, kg, seed):
    """The draws corrupt_kg(B_SIZE, False, .) consumes under ``seed`` and the negatives they give with the sampler's
    CURRENT lists, restated: per batch (mask, u_h, u_t, fb_h, fb_t), and (neg_heads, neg_tails) of the whole graph."""
    torch.manual_seed(seed)
    draws, out_h, out_t = [], [], []
    for lo in range(0, kg.n_facts, B_SIZE):
        h, t, r = (x[lo:lo + B_SIZE] for x in (kg.head_idx, kg.tail_idx, kg.relations))
        b = h.shape[0]
        mask = torch.bernoulli(samp.bern_probs[r])
        k = int(mask.sum().item())
        u_h, u_t = torch.rand((k,)), torch.rand((b - k,))
        nh, nt = h.clone(), t.clone()
        fbs = []
        for sel, u, lists, n_poss, dst in ((mask == 1, u_h, samp.possible_heads, samp.n_poss_heads, nh),
                                           (mask == 0, u_t, samp.possible_tails, samp.n_poss_tails, nt)):
            rels = r[sel].tolist()
            choice = (n_poss[r[sel]].float() * u).floor().long().tolist()
            fb = np.full(len(rels), -1, dtype=np.int64)
            corr = []
            for i, rel in enumerate(rels):
                if len(lists[rel]) == 0:
                    fb[i] = torch.randint(low=0, high=samp.n_ent, size=(1,)).item()
                    corr.append(int(fb[i]))
                else:
                    corr.append(lists[rel][choice[i]])
            dst[sel] = torch.tensor(corr, dtype=torch.long)
            fbs.append(fb)
        draws.append((mask.numpy().astype(np.uint8), u_h.numpy(), u_t.numpy(), fbs[0], fbs[1]))
        out_h.append(nh)
        out_t.append(nt)
    return draws, torch.cat(out_h), torch.cat(out_t)


def sort_lists(samp):
    for d in (samp.possible_heads, samp.possible_tails):
        for lst in d.values():
            lst.sort()


def csr(lists):
    off = np.zeros(N_REL + 1, dtype=np.int64)
    for r in range(N_REL):
        assert lists[r] == sorted(set(lists[r]))
        off[r + 1] = off[r] + len(lists[r])
    return off, np.array([e for r in range(N_REL) for e in lists[r]], dtype=np.int32)


def save_npz(path, arrays):
    """np.savez_compressed with a fixed timestamp per member: the same arrays give the same file."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    kg = make_kg(0)
    kg_val, kg_test = split(kg, 0, 400, drop_rel=EMPTY_REL), split(kg, 400, 700)
    n_empty_test = int((kg_test.relations == EMPTY_REL).sum())
    print('facts', kg.n_facts, 'validation', kg_val.n_facts, 'test', kg_test.n_facts, 'of relation 5:', n_empty_test)
    assert (kg.n_facts, kg_val.n_facts, kg_test.n_facts, n_empty_test) == (1385, 351, 300, 45)
    out = dict(n_ent=N_ENT, n_rel=N_REL, b_size=B_SIZE, empty_rel=EMPTY_REL, near=NEAR,
               val_heads=kg_val.head_idx.numpy(), val_tails=kg_val.tail_idx.numpy(), val_rels=kg_val.relations.numpy(),
               test_heads=kg_test.head_idx.numpy(), test_tails=kg_test.tail_idx.numpy(), test_rels=kg_test.relations.numpy())

    # ---- sampler -------------------------------------------------------------------------------------------
    untouched = PositionalNegativeSampler(kg_val, kg_test=kg_test)
    samp = PositionalNegativeSampler(kg_val, kg_test=kg_test)
    sort_lists(samp)
    assert samp.n_poss_heads[EMPTY_REL] == 0 and samp.n_poss_tails[EMPTY_REL] == 0
    assert int((samp.n_poss_heads == 0).sum()) == 1
    out.update(bern_probs=samp.bern_probs.numpy(), n_poss_heads=samp.n_poss_heads.numpy(),
               n_poss_tails=samp.n_poss_tails.numpy())
    out['poss_heads_offsets'], out['poss_heads_values'] = csr(samp.possible_heads)
    out['poss_tails_offsets'], out['poss_tails_values'] = csr(samp.possible_tails)
    negatives = {}
    for which, graph in (('main', kg_val), ('test', kg_test)):
        seed = SEEDS[which]
        torch.manual_seed(seed)
        ref_h, ref_t = untouched.corrupt_kg(B_SIZE, False, which=which)       # the reference as it is
        _, rep_h, rep_t = replay(untouched, graph, seed)
        assert torch.equal(ref_h, rep_h) and torch.equal(ref_t, rep_t), 'the order of draws is not the replayed one'
        torch.manual_seed(seed)
        neg_h, neg_t = samp.corrupt_kg(B_SIZE, False, which=which)            # the reference on sorted lists: recorded
        draws, rep_h, rep_t = replay(samp, graph, seed)
        assert torch.equal(neg_h, rep_h) and torch.equal(neg_t, rep_t)
        assert [len(d[0]) for d in draws][-1] == {'main': 31, 'test': 44}[which]
        n_fb = sum(int((d[3] >= 0).sum() + (d[4] >= 0).sum()) for d in draws)
        assert n_fb == (n_empty_test if which == 'test' else 0)
        out[which + '_mask'] = np.concatenate([d[0] for d in draws])
        out[which + '_k'] = np.array([int(d[0].sum()) for d in draws], dtype=np.int64)
        for i, nm in ((1, 'u_h'), (2, 'u_t'), (3, 'fb_h'), (4, 'fb_t')):
            out['%s_%s' % (which, nm)] = np.concatenate([d[i] for d in draws])
        out[which + '_neg_heads'], out[which + '_neg_tails'] = neg_h.numpy(), neg_t.numpy()
        negatives[which] = (neg_h, neg_t)
        changed = int((neg_h != graph.head_idx).sum() + (neg_t != graph.tail_idx).sum())
        print(which, 'batches', len(draws), 'changed', changed, 'of', graph.n_facts, 'fallback draws', n_fb)

    # ---- evaluator, six model kinds --------------------------------------------------------------------------
    for kind, p in CASES:
        tag = kind + ('_l1' if p == 1 else '')
        m = build_model(kind, p)
        with torch.no_grad():       # the perturbation of make_golden.py
            for prm in m.parameters():
                if prm.requires_grad:
                    prm.mul_(1.0 + 0.05 * torch.sin(torch.arange(prm.numel()).float()).view_as(prm))
        z = np.load(os.path.join(HERE, 'ref_%s.npz' % tag))
        for i, tb in enumerate(tables_of(kind, m)):
            assert np.array_equal(tb, z['table%d' % i]), (tag, i)
        ev = TripletClassificationEvaluator(m, kg_val, kg_test)
        sort_lists(ev.sampler)
        with torch.no_grad():
            torch.manual_seed(SEEDS['main'])
            ev.evaluate(B_SIZE)
            thr = ev.thresholds.clone()
            val_neg = ev.get_scores(negatives['main'][0], negatives['main'][1], kg_val.relations, B_SIZE)
            # the evaluator's own negatives were the recorded ones: its thresholds are their per-relation maxima
            for r in range(N_REL):
                sel = kg_val.relations == r
                assert thr[r] == (val_neg[sel].max() if sel.any() else val_neg.max()), (tag, r)
            torch.manual_seed(SEEDS['test'])
            acc = ev.accuracy(B_SIZE)
            pos = ev.get_scores(kg_test.head_idx, kg_test.tail_idx, kg_test.relations, B_SIZE)
            neg = ev.get_scores(negatives['test'][0], negatives['test'][1], kg_test.relations, B_SIZE)
        t = thr[kg_test.relations]
        correct = int((pos > t).sum() + (neg < t).sum())
        assert abs(acc - correct / (2 * kg_test.n_facts)) < 1e-12, (tag, acc, correct)
        near = int(((pos - t).abs() <= NEAR).sum() + ((neg - t).abs() <= NEAR).sum())
        equal = int((pos == t).sum() + (neg == t).sum())
        print('%-10s accuracy %.4f  correct %d / %d  near-threshold decisions %d (exact ties %d)'
              % (tag, acc, correct, 2 * kg_test.n_facts, near, equal))
        assert near <= 0.02 * 2 * kg_test.n_facts, (tag, near)
        out.update({tag + '_thresholds': thr.numpy(), tag + '_val_neg_scores': val_neg.numpy(), tag + '_pos_scores': pos.numpy(),
                    tag + '_neg_scores': neg.numpy(), tag + '_correct': correct, tag + '_near': near})
    path = os.path.join(HERE, 'ref_triplet.npz')
    save_npz(path, out)
    print('ref_triplet.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
