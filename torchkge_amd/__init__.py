# -*- coding: utf-8 -*-
"""torchkge_amd: MI355X-native engine for the torchkge scoring / link-prediction
hot path, behind torchkge's own Python interfaces.  See DESIGN.md."""
__version__ = '0.1.0'

from .exceptions import NotYetEvaluatedError, NotProvidedError
from .utils import MarginLoss, LogisticLoss
from .utils import l1_dissimilarity, l2_dissimilarity
from .data_structures import KnowledgeGraph, SmallKG
from .evaluation import LinkPredictionEvaluator, RelationPredictionEvaluator, clear_eval_state
from .inference import EntityInference
from .models import TransEModel, TransHModel, TransDModel, TorusEModel, TransRModel, DistMultModel, ComplExModel, RESCALModel, HolEModel, AnalogyModel, ConvKBModel
from .sampling import BernoulliNegativeSampler, UniformNegativeSampler
from .determinism import set_deterministic, is_deterministic, deterministic
from .rowgrad import set_row_gradients, is_row_gradients, row_gradients


# Names of the reference that this package does not provide at its top level: a clear error
# instead of an AttributeError, so a ported script says what to do.  RelationInference and the
# triplet-classification pair are provided by their submodules.
_NOT_PROVIDED = {
    'TripletClassificationEvaluator': 'not at the top level yet -- import it from torchkge_amd.evaluation, the path the reference\'s '
                                      'tutorial uses',
    'PositionalNegativeSampler': 'not at the top level yet -- import it from torchkge_amd.sampling, the path the reference\'s tests use',
    'RelationInference': 'not at the top level yet -- import it from torchkge_amd.inference, the module the reference keeps it in',
}


# Model classes the reference does not have.  They are served on first access and are not part of dir(torchkge_amd), which
# stays the list of the reference's eleven model classes: code that enumerates the package's model classes to mirror the
# reference (the relation-prediction and triplet-classification suites do) sees the reference's set.
_OWN_MODELS = ('RotatEModel',)
# Samplers the reference does not have: served the same way, for the same reason.
_OWN_SAMPLERS = ('FilteredNegativeSampler',)


def __getattr__(name):
    if name in _OWN_MODELS:
        from . import models
        return getattr(models, name)
    if name in _OWN_SAMPLERS:
        from . import sampling
        return getattr(sampling, name)
    if name in _NOT_PROVIDED:
        raise NotProvidedError('torchkge_amd does not provide torchkge.%s: %s (see INTEGRATION.md)' % (name, _NOT_PROVIDED[name]))
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
