"""What the ctypes bindings of the twenty-one companion libraries (``_select``, ``_f64``, ``_query``, ``_foldin``, ``_model``,
``_sets``, ``_neighbors``, ``_profile``, ``_cluster``, ``_rank``, ``_linkage``, ``_groups``, ``_kmedoids``, ``_explain``,
``_compare``, ``_diverse``, ``_operator``, ``_density``, ``_hdbscan``, ``_candidates``, ``_exemplars``) share: where libsimrank_NAME.so and include/simrank_NAME.h lie,
the lazy load with the version check, ``check``, and the layout codes of a block of an iterate.  A binding keeps its
prototypes, structures and host helpers.  The rest of what the bindings share lives elsewhere: the device scratch, the
timed stage and the band walk in ``_driver``, the scalar argument checks in ``_checks``, and the two decisions of every "a
solver's side" function (a pruned model: ``lists``; several column blocks: ``one_block``) on ``_query.SolverQueries``.
No CPU fallback: a missing library is an error.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))

# the layouts of a block of an iterate ("iterate_layout" of simrank_plan_get & co): one set of codes for every library
# that reads one, all but f64 and rank (csrc/companion.h asserts it of their headers)
PANEL_F32, ROWMAJOR_F32, PANEL_F16, ROWMAJOR_F64 = 0, 1, 2, 3


def bind(lib, prototypes, restypes):
    """argtypes / restype of every entry (restype int unless listed); AttributeError = a symbol missing from the .so."""
    for name, argtypes in prototypes.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restypes.get(name, C.c_int)
    return lib


class Companion:
    """libsimrank_<stem>.so at ``version``; ``errors`` maps a return code to the exception class that reports it
    (``error`` for the others)."""

    def __init__(self, stem, version, prototypes, restypes, error, errors=None):
        self.stem, self.version, self.prototypes, self.restypes = stem, version, prototypes, restypes
        self.error, self.errors = error, errors or {}
        self.lib_path = os.path.join(_HERE, f"libsimrank_{stem}.so")
        self.header_path = os.path.join(os.path.dirname(_HERE), "include", f"simrank_{stem}.h")
        self._lib = None

    def load(self):
        if self._lib is None:
            if not os.path.exists(self.lib_path):
                raise self.error(f"{self.lib_path} is missing: build it with `make -C simrank_amd/csrc` (no CPU fallback)")
            lib = bind(C.CDLL(self.lib_path), self.prototypes, self.restypes)
            got = getattr(lib, f"simrank_{self.stem}_version")()
            if got != self.version:
                raise self.error(f"libsimrank_{self.stem}.so version {got} != {self.version}")
            self._lib = lib
        return self._lib

    def check(self, rc: int, what: str):
        if rc != 0:
            msg = getattr(self.load(), f"simrank_{self.stem}_last_error")().decode(errors="replace")
            raise self.errors.get(rc, self.error)(f"{what} failed ({rc}): {msg}")
