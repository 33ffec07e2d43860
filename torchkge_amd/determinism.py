# -*- coding: utf-8 -*-
"""The deterministic-training switch.

With the mode ON every backward of the engine reduces its per-triple gradient rows through kge_segment_sum_ordered
(include/kge_hip_det.h): sorted runs, one writer per gradient row, a fixed summation order and no float atomic, so two
trainings from the same seed give the same tables bit for bit.  With the mode OFF (the default) every path runs as it
did before the switch existed.

The mode is on when EITHER holds:
  - the package switch is on: set_deterministic(True), the ``deterministic()`` context manager / decorator, or the
    environment variable KGE_DETERMINISTIC=1 when the package is imported;
  - torch.are_deterministic_algorithms_enabled() is true (torch.use_deterministic_algorithms(True), with or without
    warn_only).
"""
import contextlib
import os

import torch

_enabled = os.environ.get('KGE_DETERMINISTIC', '0').strip() == '1'


def set_deterministic(flag):
    """Turn the package switch on or off (torch's own flag, when set, keeps the mode on regardless)."""
    global _enabled
    _enabled = bool(flag)


def is_deterministic():
    """True when the engine's backward takes the ordered reduction: the package switch or torch's flag."""
    return _enabled or torch.are_deterministic_algorithms_enabled()


class deterministic(contextlib.ContextDecorator):
    """``with deterministic():`` / ``@deterministic()``: the package switch set to ``flag`` inside, its previous state
    restored on the way out (also after an exception).  Nests; one instance may be entered more than once."""

    def __init__(self, flag=True):
        self.flag = bool(flag)
        self._prev = []

    def __enter__(self):
        self._prev.append(_enabled)
        set_deterministic(self.flag)
        return self

    def __exit__(self, *exc):
        set_deterministic(self._prev.pop())
        return False
