"""Stand-ins for the device that CPU tests of a kept model's host logic share: ``HostOps`` keeps ``HipOps``'s memory calls
on host memory, the ``Spec`` / ``Tables`` stubs are what an estimator's argument checks look at, and ``boom`` marks a call
that must not happen."""
import ctypes

import numpy as np


def boom(*a, **k):
    raise AssertionError("the device was touched")


class HostOps:
    """``HipOps``'s memory calls on host memory; ``live`` maps every block that was not freed."""
    stream = None

    def __init__(self):
        self.live = {}

    def _malloc(self, nbytes):
        buf = np.zeros(max(16, int(nbytes)), dtype=np.uint8)
        self.live[buf.ctypes.data] = buf
        return buf.ctypes.data

    def _free(self, ptr):
        del self.live[ptr]

    def h2d(self, ptr, host):
        ctypes.memmove(ptr, host.ctypes.data, host.nbytes)

    def d2h(self, host, ptr, nbytes=None):
        ctypes.memmove(host.ctypes.data, ptr, host.nbytes if nbytes is None else nbytes)

    def put(self, host):
        ptr = self._malloc(host.nbytes)
        self.h2d(ptr, host)
        return ptr

    def synchronize(self):
        pass


class StubCsr:
    rowptr, col = np.array([0, 2, 2, 3], dtype=np.int32), np.array([2, 0, 1], dtype=np.int32)


class StubSpec:
    """A side of three nodes whose arrays no argument check reads."""
    csr, rowscale, storage, apriori, evidence_from = StubCsr, np.array([0.5, 0.0, 1.0]), "f32", None, None


class StubTables:
    """Tables of three nodes and two kept neighbours that hold no memory."""
    n, k, ids, nbytes = 3, 2, 1, 3 * 2 * 12 + 3 * 8

    def free(self):
        self.ids = None


class RingSpec:
    """A side of n nodes on a ring (node i's one in-neighbour is i + 1), unit scales, no evidence, no prior."""

    def __init__(self, n):
        from simrank_amd.ingest import CSR
        self.csr = CSR(n, n, np.arange(n + 1, dtype=np.int32), ((np.arange(n) + 1) % n).astype(np.int32), np.ones(n))
        self.rowscale, self.coef, self.lbd = np.ones(n), 0.8, 0.0
        self.evidence_from, self.apriori, self.storage = None, None, "f32"
