# -*- coding: utf-8 -*-
from .interfaces import Model, TranslationModel, BilinearModel, EntityCandidates
from .translation import TransEModel, TransHModel, TransDModel, TorusEModel, TransRModel, RotatEModel
from .bilinear import DistMultModel, ComplExModel, RESCALModel, HolEModel, AnalogyModel
from .deep import ConvKBModel
