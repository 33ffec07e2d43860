# -*- coding: utf-8 -*-
"""Generate the training-loop golden fixture in this directory by RUNNING THE REAL REFERENCE
(torchkge v0.17.7 imported from /root/reference, CPU).  Run in the build container only (the
reference does not exist on the GPU box):

    python tests/golden/make_golden_trainer.py

Output (committed): tests/golden/ref_trainer.npz, written with fixed archive timestamps so that a
second run gives the same bytes.

The loop is the reference's own ``Trainer.run`` (utils/training.py:169-188) without its line 179
(``data_loader.get_counter_examples()`` before the first iteration raises AttributeError): the
reference's ``TrainDataLoader`` ('bern', host tensors), ``Trainer.process_batch`` per batch, the
mean of the step losses per epoch, ``model.normalize_parameters()`` after every epoch.

Graph: make_golden.make_kg(0) (1,385 facts, 300 entities, 7 relations).  Batch 128 (the last batch
has 105 facts), three epochs, torch.optim.SGD with lr = 0.01.  Cases: TransE-L2 with
MarginLoss(0.5), DistMult with LogisticLoss, ComplEx with BinaryCrossEntropyLoss, all d = 16.

Per case the loop runs twice from the same seeds: in fp32, and with the model cast to double
after construction.  Stored: the graph, the initial tables, the negatives of every epoch (of both
runs: they must be equal, asserted here and again by tests/test_trainer_host.py), the mean losses
and final tables of both runs and, for the margin case, the smallest |margin - p + n| any pair met
in the fp64 run -- asserted >= 1e-4 so that no hinge can flip inside fp32 noise (further seeds are
tried if a later change moves it).
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
from torchkge.models import TransEModel, DistMultModel, ComplExModel  # noqa: E402
from torchkge.utils.losses import MarginLoss, LogisticLoss, BinaryCrossEntropyLoss  # noqa: E402
from torchkge.utils.training import Trainer, TrainDataLoader  # noqa: E402
from make_golden import make_kg, N_ENT, N_REL  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
assert torchkge.__version__ == '0.17.7'
DIM, B_SIZE, N_EPOCHS, LR, MARGIN, MIN_HINGE = 16, 128, 3, 0.01, 0.5, 1e-4
CASES = {
    'transe': (lambda: TransEModel(DIM, N_ENT, N_REL, dissimilarity_type='L2'), lambda: MarginLoss(MARGIN),
               ('ent_emb', 'rel_emb')),
    'distmult': (lambda: DistMultModel(DIM, N_ENT, N_REL), LogisticLoss, ('ent_emb', 'rel_emb')),
    'complex': (lambda: ComplExModel(DIM, N_ENT, N_REL), BinaryCrossEntropyLoss,
                ('re_ent_emb', 'im_ent_emb', 're_rel_emb', 'im_rel_emb')),
}


def save_npz(path, arrays):
    """np.savez_compressed with a fixed timestamp per member: the same arrays give the same file."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


class Recording(object):
    """The criterion, with the smallest |margin - p + n| it has seen noted on the way."""

    def __init__(self, criterion, margin):
        self.criterion, self.margin, self.min_hinge = criterion, margin, float('inf')

    def __call__(self, p, n):
        if self.margin is not None:
            self.min_hinge = min(self.min_hinge, float((self.margin - p.detach() + n.detach()).abs().min()))
        return self.criterion(p, n)


def tables(model, names):
    return [getattr(model, nm).weight.detach().clone().numpy() for nm in names]


def run(kg, case, seed, double):
    make_model, make_criterion, names = CASES[case]
    torch.manual_seed(seed)
    model = make_model()
    if double:
        model = model.double()
    init = tables(model, names)
    criterion = Recording(make_criterion(), MARGIN if case == 'transe' else None)
    trainer = Trainer(model, criterion, kg, N_EPOCHS, B_SIZE, torch.optim.SGD(model.parameters(), lr=LR),
                      sampling_type='bern', use_cuda=None)
    torch.manual_seed(seed + 1000)
    loader = TrainDataLoader(kg, batch_size=B_SIZE, sampling_type='bern', use_cuda=None)
    negs, losses = [], []
    for _ in range(N_EPOCHS):
        sum_ = 0
        for i, batch in enumerate(loader):
            sum_ += trainer.process_batch(batch)
        ce = loader.get_counter_examples()
        negs.append((ce.head_idx.clone().numpy(), ce.tail_idx.clone().numpy()))
        losses.append(sum_ / len(loader))
        model.normalize_parameters()
    assert i == len(loader) - 1 == kg.n_facts // B_SIZE and len(batch['h']) == kg.n_facts % B_SIZE == 105
    return dict(init=init, final=tables(model, names), losses=np.array(losses, dtype=np.float64),
                nh=np.stack([x[0] for x in negs]), nt=np.stack([x[1] for x in negs]), min_hinge=criterion.min_hinge)


def main():
    kg = make_kg(0)
    assert (kg.n_facts, kg.n_ent, kg.n_rel) == (1385, N_ENT, N_REL)
    out = dict(n_ent=N_ENT, n_rel=N_REL, dim=DIM, b_size=B_SIZE, n_epochs=N_EPOCHS, lr=LR, margin=MARGIN,
               min_hinge_bound=MIN_HINGE, heads=kg.head_idx.numpy(), tails=kg.tail_idx.numpy(), rels=kg.relations.numpy())
    for case in CASES:
        for seed in range(20):
            r32, r64 = run(kg, case, seed, False), run(kg, case, seed, True)
            if case != 'transe' or r64['min_hinge'] >= MIN_HINGE:
                break
            print(case, 'seed', seed, 'smallest hinge argument', r64['min_hinge'], '-- next seed')
        assert np.array_equal(r32['nh'], r64['nh']) and np.array_equal(r32['nt'], r64['nt']), case
        assert all(np.array_equal(a, b.astype(np.float32)) for a, b in zip(r32['init'], r64['init'])), case
        assert all(t.dtype == np.float32 for t in r32['final']) and all(t.dtype == np.float64 for t in r64['final'])
        out[case + '_seed'] = seed
        out[case + '_nh32'], out[case + '_nt32'] = r32['nh'].astype(np.int32), r32['nt'].astype(np.int32)
        out[case + '_nh64'], out[case + '_nt64'] = r64['nh'].astype(np.int32), r64['nt'].astype(np.int32)
        out[case + '_loss32'], out[case + '_loss64'] = r32['losses'], r64['losses']
        for i, (a, f32, f64) in enumerate(zip(r32['init'], r32['final'], r64['final'])):
            out['%s_init%d' % (case, i)], out['%s_final32_%d' % (case, i)], out['%s_final64_%d' % (case, i)] = a, f32, f64
        dist = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32['final'], r64['final']))
        changed = int((r32['nh'] != kg.head_idx.numpy()).sum() + (r32['nt'] != kg.tail_idx.numpy()).sum())
        print('%-9s seed %d  mean losses %s  |final32 - final64| %.3g  corrupted %d of %d'
              % (case, seed, np.array2string(r64['losses'], precision=5), dist, changed, N_EPOCHS * kg.n_facts))
        if case == 'transe':
            assert r64['min_hinge'] >= MIN_HINGE
            out['transe_min_hinge'] = r64['min_hinge']
            print('          smallest |margin - p + n| of the fp64 run: %.3g' % r64['min_hinge'])
    path = os.path.join(HERE, 'ref_trainer.npz')
    save_npz(path, out)
    print('ref_trainer.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
