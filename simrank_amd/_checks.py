"""The two scalar predicates the argument checks of the companion bindings share (``_query``, ``_explain``, ``_groups``,
``_kmedoids``, ``_linkage``, ``_profile``, ``_cluster``, ``_density``).  Every message stays with the check that raises it, except the one
message that three checks share word for word (``finite``).  Nothing here touches a device.
"""
from __future__ import annotations

import math
import numbers

import numpy as np


def is_int(x) -> bool:
    """An integer of any type that is not a bool."""
    return isinstance(x, numbers.Integral) and not isinstance(x, (bool, np.bool_))


def is_finite_real(x) -> bool:
    """One finite real number: a 0-d array holds one; a bool is none, nor is an int too large for a float."""
    if isinstance(x, np.ndarray) and x.ndim == 0:
        x = x[()]
    try:
        return not isinstance(x, (bool, np.bool_)) and isinstance(x, numbers.Real) and math.isfinite(float(x))
    except OverflowError:
        return False


def finite(x, what) -> float:
    """``x`` as a float: a threshold of ``components``, the floor of ``linkage``, the ``t`` of ``cut``.  ValueError for
    anything that is no finite number."""
    if isinstance(x, np.ndarray) and x.ndim == 0:
        x = x[()]                                            # (the message shows the number the array holds)
    if not is_finite_real(x):
        raise ValueError(f"{what} must be a finite number, not {x!r}")
    return float(x)
