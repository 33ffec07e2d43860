# -*- coding: utf-8 -*-
"""``TrainDataLoader`` and ``Trainer`` with the reference's interface (torchkge/utils/training.py:15-200), so that the
reference's training tutorial runs with the import changed:

    from torchkge_amd.utils.training import Trainer
    trainer = Trainer(model, criterion, kg_train, n_epochs, batch_size, optimizer, sampling_type='bern', use_cuda='all')
    trainer.run()

What is the engine's own:
  * with ``fused=True`` (the default) a criterion of ``utils/losses.py`` is replaced by its fused counterpart
    (``utils/fused_losses.py``: loss and gradients from one kge_pair_loss, finite in saturation); any other criterion
    takes the generic path -- forward, ``criterion(p, n)``, backward, step;
  * an optimizer of ``torchkge_amd.optim`` makes every step run inside ``row_gradients()``;
  * ``sync_free=True``: ``run()`` reads nothing back -- the sampler draws without its host read, the steps add their loss
    into one device float per epoch, ``epoch_losses`` fetches the epoch sums on first access;
  * ``sampler=``: any object with a ``corrupt_kg`` instead of the two built-in samplers;
  * ``n_neg=K``: K negatives per fact -- the loader hands every batch its ``K * B_b`` negatives in tile order and
    ``Model.forward`` repeats the positives; a criterion of ``utils/group_losses.py`` (self-adversarial, sampled softmax)
    weighs the K negatives of a fact against each other in one kge_group_loss, any pairwise criterion sees K pairs per fact;
  * ``trainer.grouped_forward = True`` (an attribute, off by default): the scores come from
    ``Model.forward_grouped`` -- a fact's rows gathered once for its K negatives, K + 3 instead of 3 (K + 1) gradient rows
    per fact for TransE -- with the bits of ``Model.forward``;
  * ``trainer.regularizer = N3Regularizer(...)`` (an attribute of all three trainers, None by default): an embedding
    regularizer of ``utils/regularizers.py`` penalises the rows of the batch's facts (not the negatives; K-vs-all: the key's
    entity and relation row); its gradient rows are sparse inside ``row_gradients()``, so the row optimizers keep working,
    and the penalty is part of ``epoch_losses``;
  * ``get_counter_examples()`` is None before ``run()`` and the last epoch's negatives after it (the reference's
    ``run`` asks its loader for them before the first iteration and raises).

``OneVsAllTrainer`` is the engine's own: the same epochs without a sampler, on ``model.one_vs_all_loss`` (the softmax
cross-entropy over all entities of torchkge_amd.utils.one_vs_all; DistMultModel and ComplExModel).  ``KvsAllTrainer``
is its multi-label counterpart: the distinct keys of the graph as queries, ``model.k_vs_all_loss`` (binary cross-entropy
over all entities against each key's answer set, torchkge_amd.utils.k_vs_all) as the criterion.

The models live on the GPU: ``use_cuda`` is 'all' or 'batch'."""
import contextlib

import torch

from .. import optim
from ..data_structures import SmallKG
from ..models.interfaces import Model
from ..rowgrad import row_gradients
from ..sampling import BernoulliNegativeSampler, UniformNegativeSampler
from .data import get_n_batches
from .fused_losses import fused_for
from .group_losses import _GroupCriterion


class TrainDataLoader:
    """Batches of true and negatively sampled facts: dicts with the keys ``h, t, r, nh, nt``, the last one short.  Every
    ``__iter__`` corrupts the whole graph anew (``sampler.corrupt_kg``).

    ``use_cuda``: None (host tensors), 'batch' (each batch is moved when it is returned) or 'all' (the graph's vectors
    move once, the negatives are drawn on the device and the batches are slices: nothing goes through the host).
    ``sampler``: an object with ``corrupt_kg(batch_size, use_cuda, on_device=...)``; ``sampling_type`` ('unif' / 'bern')
    is then ignored.  ``sync_free=True`` sets the sampler's ``sync_free`` flag.

    ``n_neg``: negatives per fact.  Above 1 the sampler's ``corrupt_kg`` is asked for ``n_neg=`` (a sampler with the old
    signature serves ``n_neg=1`` only) and batch b of B_b facts gets the ``n_neg * B_b`` negatives of its own block, in
    the tile order ``Model.forward`` expects: ``nh[k * B_b + i]`` is the k-th negative of the batch's fact i."""

    def __init__(self, kg, batch_size, sampling_type, use_cuda=None, *, sampler=None, sync_free=False, n_neg=1):
        self.h, self.t, self.r = kg.head_idx, kg.tail_idx, kg.relations
        self.use_cuda = use_cuda
        self.b_size = batch_size
        if int(n_neg) < 1:
            raise ValueError('n_neg must be at least 1, got %r' % (n_neg,))
        self.n_neg = int(n_neg)
        self.iterator = None
        if sampler is not None:
            self.sampler = sampler
        elif sampling_type == 'unif':
            self.sampler = UniformNegativeSampler(kg)
        elif sampling_type == 'bern':
            self.sampler = BernoulliNegativeSampler(kg)
        else:
            raise ValueError("sampling_type is 'unif' or 'bern', got %r" % (sampling_type,))
        if sync_free:
            self.sampler.sync_free = True
        self.tmp_cuda = use_cuda in ['batch', 'all']
        if use_cuda == 'all':
            self.h, self.t, self.r = self.h.cuda(), self.t.cuda(), self.r.cuda()

    def __len__(self):
        return get_n_batches(len(self.h), self.b_size)

    def __iter__(self):
        self.iterator = TrainDataLoaderIter(self)
        return self.iterator

    def get_counter_examples(self):
        """``SmallKG(nh, nt, r)`` of the latest ``__iter__``; None before the first.  With ``n_neg > 1`` the relations are
        tiled batch by batch to match the negatives' blocks."""
        if self.iterator is None:
            return None
        it = self.iterator
        r = it.r
        if self.n_neg > 1:
            r = torch.cat([r[lo:lo + self.b_size].repeat(self.n_neg) for lo in range(0, len(r), self.b_size)])
        return SmallKG(it.nh, it.nt, r)


class TrainDataLoaderIter:
    def __init__(self, loader):
        self.h, self.t, self.r = loader.h, loader.t, loader.r
        self.n_neg = loader.n_neg
        more = {'n_neg': self.n_neg} if self.n_neg > 1 else {}      # (a sampler with the old signature serves n_neg = 1)
        if loader.use_cuda == 'all':
            self.nh, self.nt = loader.sampler.corrupt_kg(loader.b_size, True, on_device=True, **more)
        else:
            self.nh, self.nt = loader.sampler.corrupt_kg(loader.b_size, loader.tmp_cuda, **more)
        if loader.use_cuda:
            self.nh, self.nt = self.nh.cuda(), self.nt.cuda()
        self.use_cuda = loader.use_cuda
        self.b_size = loader.b_size
        self.n_batches = get_n_batches(len(self.h), self.b_size)
        self.current_batch = 0

    def __next__(self):
        if self.current_batch == self.n_batches:
            raise StopIteration
        sl = slice(self.current_batch * self.b_size, (self.current_batch + 1) * self.b_size)
        self.current_batch += 1
        if self.n_neg > 1:      # the batch's own block of n_neg * B_b negatives (the last batch is short)
            nsl = slice(self.n_neg * sl.start, self.n_neg * min(sl.stop, len(self.h)))
        else:
            nsl = sl
        batch = {'h': self.h[sl], 't': self.t[sl], 'r': self.r[sl], 'nh': self.nh[nsl], 'nt': self.nt[nsl]}
        if self.use_cuda == 'batch':
            batch = {k: v.cuda() for k, v in batch.items()}
        return batch

    def __iter__(self):
        return self


class _EpochLoop:
    """The epochs of the three trainers, written once: ``run()`` and ``epoch_losses``.  A trainer supplies ``_step(batch,
    acc=None)`` -- one training step, its loss as a device scalar, also added to the device float ``acc`` when given --
    and the hooks below.  It reads ``model``, ``n_epochs``, ``sync_free`` and ``verbose`` of the instance."""

    _epoch_sums = None          # sync_free: (device vector of the epochs' loss sums, batches per epoch)

    def _prepare(self):
        """Called by every ``run()`` behind ``model.cuda()``: builds and uploads what the batches are cut from, once --
        a later ``run()`` finds it kept."""

    def _batches(self):
        """The batches of one epoch, as ``_step`` takes them."""
        raise NotImplementedError

    def _n_batches(self):
        """The divisor of an epoch's loss sum (after ``_prepare``)."""
        raise NotImplementedError

    def _host_loss(self, batch):
        """One step without ``sync_free``; its loss as a Python float (the step's one host read)."""
        return self._step(batch).item()

    def _after_epoch(self):
        """Called behind ``model.normalize_parameters()``."""

    def run(self):
        self.model.cuda()
        self._prepare()
        epochs = range(self.n_epochs)
        bar = None
        if self.verbose:
            try:
                from tqdm.autonotebook import tqdm
                epochs = bar = tqdm(epochs, unit='epoch')
            except ImportError:
                pass
        n_batches = self._n_batches()
        self._epoch_losses, self._epoch_sums = [], None
        if self.sync_free:
            device = next(self.model.parameters()).device
            self._epoch_sums = (torch.zeros(self.n_epochs, dtype=torch.float32, device=device), n_batches)
        for epoch in epochs:
            if self.sync_free:
                acc = self._epoch_sums[0][epoch]        # a view: the steps add into the vector's own element
                for batch in self._batches():
                    self._step(batch, acc)
            else:
                sum_ = 0
                for batch in self._batches():
                    sum_ += self._host_loss(batch)
                self._epoch_losses.append(sum_ / n_batches)
                if bar is not None:
                    bar.set_description('Epoch {} | mean loss: {:.5f}'.format(epoch + 1, self._epoch_losses[-1]))
            self.model.normalize_parameters()
            self._after_epoch()

    @property
    def epoch_losses(self):
        """The mean step loss of every epoch of the last ``run()``, as Python floats.  After a ``sync_free`` run the
        first access reads the epoch sums back (one copy)."""
        if self._epoch_sums is not None:
            sums, n_batches = self._epoch_sums
            self._epoch_losses, self._epoch_sums = [s / n_batches for s in sums.cpu().tolist()], None
        return self._epoch_losses


class Trainer(_EpochLoop):
    """The reference's training procedure: per epoch a fresh corruption of ``kg_train``, one step per batch,
    ``model.normalize_parameters()``; the mean loss of every epoch is kept in ``epoch_losses``.

    ``grouped_forward`` is an attribute, False by default (the constructor's parameters are those of the release before
    it): set ``trainer.grouped_forward = True`` before ``run()`` and every batch is scored with
    ``model.forward_grouped`` instead of ``model.forward`` -- the same score bits, fewer gathered and emitted rows (models
    and widths the grouped kernels do not serve take ``forward`` inside it).  That path needs negatives that differ from
    their fact in at most one of head and tail.  The package's own samplers guarantee it and are not checked.  A
    ``sampler=`` from elsewhere is checked on every step, one host read each -- unless ``sync_free``, which reads nothing
    back: THEN THE CONTRACT IS THE CALLER'S, and a negative that breaks it is scored as (negative head, relation, the
    fact's tail)."""

    grouped_forward = False     # True: Model.forward_grouped scores the batches (set it on the instance)
    regularizer = None          # an embedding regularizer of utils/regularizers.py (set it on the instance)

    def __init__(self, model, criterion, kg_train, n_epochs, batch_size, optimizer, sampling_type='bern', use_cuda=None,
                 *, fused=True, sync_free=False, sampler=None, verbose=True, n_neg=1):
        if use_cuda not in ('all', 'batch'):
            raise ValueError("Trainer: use_cuda must be 'all' or 'batch', got %r -- the engine's models live on the GPU, "
                             "there is no CPU training path" % (use_cuda,))
        self.model = model
        self.criterion = criterion
        self.kg_train = kg_train
        self.use_cuda = use_cuda
        self.n_epochs = n_epochs
        self.optimizer = optimizer
        self.sampling_type = sampling_type
        self.batch_size = batch_size
        self.n_triples = len(kg_train)
        self.fused = fused
        self.sync_free = sync_free
        self.sampler = sampler
        self.verbose = verbose
        self.counter_examples = None
        if int(n_neg) < 1:
            raise ValueError('Trainer: n_neg must be at least 1, got %r' % (n_neg,))
        self.n_neg = int(n_neg)
        own_sampler = sampler is None or type(sampler).__module__ == BernoulliNegativeSampler.__module__
        self._check_negatives = not own_sampler and not sync_free      # grouped_forward: one host read per step
        self._grouped = isinstance(criterion, _GroupCriterion)
        if self._grouped:
            if criterion.n_neg is None:
                criterion.n_neg = self.n_neg
            elif criterion.n_neg != self.n_neg:
                raise ValueError('Trainer: the criterion groups %d negatives per fact, the Trainer draws %d'
                                 % (criterion.n_neg, self.n_neg))
        self._fused_criterion = fused_for(criterion) if fused else None
        self._row_mode = isinstance(optimizer, (optim.RowSGD, optim.RowAdagrad, optim.RowAdam))
        self._loader = None
        self._epoch_losses = []

    def _step(self, batch, acc=None):
        """One training step; the loss as a device scalar, also added to the device float ``acc`` when given."""
        with row_gradients() if self._row_mode else contextlib.nullcontext():
            self.optimizer.zero_grad()
            if self.grouped_forward:
                p, n = self.model.forward_grouped(batch['h'], batch['t'], batch['r'], batch['nh'], batch['nt'],
                                                  check=self._check_negatives)
            else:
                p, n = self.model(batch['h'], batch['t'], batch['r'], batch['nh'], batch['nt'])
            if self._fused_criterion is not None:
                loss = self._fused_criterion(p, n, acc)
            elif self._grouped:
                loss = self.criterion(p, n, acc)
            else:
                loss = self.criterion(p, n)
                if acc is not None:
                    acc.add_(loss.detach())
            if self.regularizer is not None:    # the batch's facts; the negatives are not penalised
                loss = loss + self.regularizer(self.model, (batch['h'], batch['t']), (batch['r'],), acc)
            loss.backward()
            self.optimizer.step()
        return loss.detach()

    def process_batch(self, current_batch):
        """One step on a batch of the loader; its loss as a Python float (the step's one host read)."""
        return self._step(current_batch).item()

    def _host_loss(self, batch):
        return self.process_batch(batch)

    def _prepare(self):
        if isinstance(self.criterion, torch.nn.Module):
            self.criterion.cuda()
        if self._loader is None:        # kept: a later run() uploads nothing again
            self._loader = TrainDataLoader(self.kg_train, batch_size=self.batch_size, sampling_type=self.sampling_type,
                                           use_cuda=self.use_cuda, sampler=self.sampler, sync_free=self.sync_free,
                                           n_neg=self.n_neg)

    def _batches(self):
        return self._loader     # every iteration corrupts the graph anew

    def _n_batches(self):
        return len(self._loader)

    def _after_epoch(self):
        self.counter_examples = self._loader.get_counter_examples()

    def get_counter_examples(self):
        """The counter-examples of the last epoch as a ``SmallKG``; None before ``run()``."""
        return self.counter_examples


class _DenseGradientTrainer(_EpochLoop):
    """What OneVsAllTrainer and KvsAllTrainer share: the constructor and its checks.  ``_REGIME`` names the regime in the
    messages, ``_LOSS`` the model method it trains on."""

    def __init__(self, model, kg_train, n_epochs, batch_size, optimizer, label_smoothing=0.0, side='both', use_cuda='all',
                 *, sync_free=False, verbose=True):
        name = type(self).__name__
        if use_cuda not in ('all', 'batch'):
            raise ValueError("%s: use_cuda must be 'all' or 'batch', got %r -- the engine's models live on the "
                             "GPU, there is no CPU training path" % (name, use_cuda))
        if side not in ('both', 'tail', 'head'):
            raise ValueError("%s: side is 'both', 'tail' or 'head', got %r" % (name, side))
        if isinstance(optimizer, (optim.RowSGD, optim.RowAdagrad, optim.RowAdam)):
            raise ValueError('%s: %s updates the rows of a sparse row gradient, but the %s gradient of '
                             'an entity table is dense (every entity is a candidate of every query); use a torch.optim '
                             'optimizer' % (name, type(optimizer).__name__, self._REGIME))
        if getattr(type(model), self._LOSS) is getattr(Model, self._LOSS):
            getattr(model, self._LOSS)(None, None, None, None)      # raises NotImplementedError, naming those that have it
        self.model = model
        self.kg_train = kg_train
        self.use_cuda = use_cuda
        self.n_epochs = n_epochs
        self.optimizer = optimizer
        self.batch_size = batch_size
        self.label_smoothing = label_smoothing
        self.side = side
        self.n_triples = len(kg_train)
        self.sync_free = sync_free
        self.verbose = verbose
        self._epoch_losses = []

    regularizer = None          # an embedding regularizer of utils/regularizers.py (set it on the instance)

    def _loss(self, batch):
        raise NotImplementedError

    def _penalised(self, batch):
        """(entity id vectors, relation id vectors) of a batch that ``regularizer`` penalises."""
        raise NotImplementedError

    def _step(self, batch, acc=None):
        """One training step; the loss as a device scalar, also added to the device float ``acc`` when given."""
        self.optimizer.zero_grad()
        loss = self._loss(batch)
        if acc is not None:
            acc.add_(loss.detach())
        if self.regularizer is not None:
            loss = loss + self.regularizer(self.model, *self._penalised(batch), acc)
        loss.backward()
        self.optimizer.step()
        return loss.detach()


class OneVsAllTrainer(_DenseGradientTrainer):
    """1-vs-all training of a model with ``one_vs_all_loss`` (DistMultModel, ComplExModel): per batch the softmax
    cross-entropy of the true tail / head among ALL entities (torchkge_amd.utils.one_vs_all), without the (B, N) score
    matrix.  There is no sampler and no criterion; the epochs are ``Trainer``'s -- the facts in their order, the last
    batch short, ``model.normalize_parameters()`` after each, the mean step loss in ``epoch_losses`` (``sync_free=True``:
    the steps add into one device float per epoch, read back on first access).

    The entity tables' gradient is dense in this regime, so the row-wise optimizers of ``torchkge_amd.optim`` are
    refused: use a ``torch.optim`` optimizer."""

    _REGIME, _LOSS = '1-vs-all', 'one_vs_all_loss'
    _facts = None

    def _loss(self, batch):
        return self.model.one_vs_all_loss(batch[0], batch[1], batch[2], side=self.side, label_smoothing=self.label_smoothing,
                                          reduction='mean')

    def _penalised(self, batch):
        return (batch[0], batch[1]), (batch[2],)

    def _prepare(self):
        if self._facts is None:        # kept: a later run() uploads nothing again
            kg = self.kg_train
            self._facts = (kg.head_idx, kg.tail_idx, kg.relations)
            if self.use_cuda == 'all':
                self._facts = tuple(x.cuda() for x in self._facts)

    def _n_batches(self):
        return get_n_batches(len(self._facts[0]), self.batch_size)

    def _batches(self):
        h, t, r = self._facts
        for b in range(self._n_batches()):
            sl = slice(b * self.batch_size, (b + 1) * self.batch_size)
            batch = (h[sl], t[sl], r[sl])
            yield tuple(x.cuda() for x in batch) if self.use_cuda == 'batch' else batch


class KvsAllTrainer(_DenseGradientTrainer):
    """K-vs-all training of a model with ``k_vs_all_loss`` (DistMultModel, ComplExModel): a query is a distinct key of
    the training graph -- (h, r) on the tail side, (t, r) on the head side -- its label the whole set of known answers,
    the criterion a binary cross-entropy with logits over ALL entities (torchkge_amd.utils.k_vs_all), without the (B, N)
    score, label or gradient matrix.

    The labels are two ``FilterIndex``es built once from ``kg_train``'s own triples (``from_triples_torch`` with the
    bounds n_ent, n_rel, n_ent): (h, r) -> tails and (t, r) -> heads.  An epoch walks the distinct keys of the chosen
    side(s) in index order -- ``side='both'``: the tail side's batches, then the head side's -- in batches of
    ``batch_size`` keys, the last of a side short; a batch's segments are slices of the index's ``offsets`` and its
    answers are read in place from the index's ``targets``.  There is no sampler and no criterion;
    ``model.normalize_parameters()`` runs after each epoch, ``epoch_losses`` holds the mean step loss
    (``sync_free=True``: the steps add into one device float per epoch, read back on first access).

    The entity tables' gradient is dense in this regime, so the row-wise optimizers of ``torchkge_amd.optim`` are
    refused: use a ``torch.optim`` optimizer."""

    _REGIME, _LOSS = 'K-vs-all', 'k_vs_all_loss'
    _indexes = None             # {'tail': FilterIndex (h, r) -> tails, 'head': FilterIndex (t, r) -> heads}
    _targets = None             # the indexes' answer lists on the GPU

    @staticmethod
    def key_batches(index, batch_size):
        """The batches of one side: ``(ent_idx, r_idx, seg_lo, seg_hi)`` of the distinct keys ``index.keys`` in index
        order, ``batch_size`` at a time -- pure index arithmetic on the index's own tensors, no lookup kernel."""
        from ..filter_index import KEY2_SPAN
        keys, offsets = index.keys, index.offsets
        for b in range(get_n_batches(index.n_keys, batch_size)):
            lo, hi = b * batch_size, min((b + 1) * batch_size, index.n_keys)
            k = keys[lo:hi]
            yield k // KEY2_SPAN, k % KEY2_SPAN, offsets[lo:hi], offsets[lo + 1:hi + 1]

    def _sides(self):
        return ('tail', 'head') if self.side == 'both' else (self.side,)

    def n_batches(self):
        """Steps of one epoch (after the indexes exist)."""
        return sum(get_n_batches(self._indexes[s].n_keys, self.batch_size) for s in self._sides())

    def _n_batches(self):
        return max(self.n_batches(), 1)

    def _prepare(self):
        if self._indexes is not None:       # kept: a later run() builds and uploads nothing again
            return
        from ..filter_index import FilterIndex
        kg = self.kg_train
        device = next(self.model.parameters()).device if self.use_cuda == 'all' else torch.device('cpu')
        h, t, r = kg.head_idx, kg.tail_idx, kg.relations
        self._indexes = {
            'tail': FilterIndex.from_triples_torch(h, r, t, device, kg.n_ent, kg.n_rel, kg.n_ent),
            'head': FilterIndex.from_triples_torch(t, r, h, device, kg.n_ent, kg.n_rel, kg.n_ent)}
        self._targets = {s: ix.targets.cuda() for s, ix in self._indexes.items()}     # 'batch': the one upload of the labels

    def _batches(self):
        for side in self._sides():
            for batch in self.key_batches(self._indexes[side], self.batch_size):
                if self.use_cuda == 'batch':
                    batch = tuple(x.cuda() for x in batch)
                yield side, batch

    def _loss(self, batch):
        side, (e, r, seg_lo, seg_hi) = batch
        return self.model.k_vs_all_loss(e, r, (seg_lo, seg_hi, self._targets[side]), side,
                                        label_smoothing=self.label_smoothing, reduction='mean')

    def _penalised(self, batch):
        """The key's entity row and relation row."""
        return (batch[1][0],), (batch[1][1],)
