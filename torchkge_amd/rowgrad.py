# -*- coding: utf-8 -*-
"""The row-gradient switch.

With the mode ON the backward of every scoring function returns the gradient of an embedding table as an UNCOALESCED
``torch.sparse_coo_tensor`` of the table's shape: the ids the row reduction would have used (``cat(h, t)`` for entity
tables, ``r`` for relation tables) and the matching per-triple gradient rows -- no sort, no sum, no ``zeros_like(table)``.
The optimizers of torchkge_amd.optim coalesce those rows and update the touched rows only (kge_rows_coalesce and the
kge_row_* kernels, include/kge_hip_rows.h); torch's SGD, Adagrad and SparseAdam accept them as they are.  Gradients
that are not row-shaped (RESCAL's rel_mat, TransR's proj_mat, ConvKB's layers) stay dense.  With the mode OFF (the
default) every path runs as it did before the switch existed.

The mode is read when the FORWARD runs: a loss built inside ``row_gradients()`` gives row gradients wherever its
``.backward()`` is called.  It is on after set_row_gradients(True), inside the ``row_gradients()`` context manager /
decorator, or with the environment variable KGE_ROW_GRADIENTS=1 when the package is imported.
"""
import contextlib
import os

_enabled = os.environ.get('KGE_ROW_GRADIENTS', '0').strip() == '1'


def set_row_gradients(flag):
    """Turn the package switch on or off."""
    global _enabled
    _enabled = bool(flag)


def is_row_gradients():
    """True when a forward that runs now will give row gradients in its backward."""
    return _enabled


class row_gradients(contextlib.ContextDecorator):
    """``with row_gradients():`` / ``@row_gradients()``: the package switch set to ``flag`` inside, its previous state
    restored on the way out (also after an exception).  Nests; one instance may be entered more than once."""

    def __init__(self, flag=True):
        self.flag = bool(flag)
        self._prev = []

    def __enter__(self):
        self._prev.append(_enabled)
        set_row_gradients(self.flag)
        return self

    def __exit__(self, *exc):
        set_row_gradients(self._prev.pop())
        return False
