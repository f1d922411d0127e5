#!/usr/bin/env python3
"""How much of leg 1's transposed product a triangle-form leg 2 never reads, on the CPU (no GPU, no library).

    python tools/leg1_dead_units.py [workload ...]        (default: pl32768d32 pl32768 pl65536 er8192)

Restates planprep.hip in NumPy: the stable ascending-length order, two refinement passes by (length, first referencing
row), then first_block[P] = min over the panel's 32 nodes of first(i) / 128.  Prints, per workload and for both orders,
the share of (128-row block, 32-column panel) units with block < first_block[panel] and the share of the pattern's
entries whose (block, panel) products fall into them.  profiles/leg1_skip_ab.md quotes this output."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simrank_amd import ingest, synth  # noqa: E402


def first_ref(n, rows, cols, inv):
    """first[i] = smallest position (under inv) of a row whose list holds i; n: nobody."""
    first = np.full(n, n, dtype=np.int64)
    np.minimum.at(first, cols, inv[rows])
    return first


def orders(rowptr, col):
    n = len(rowptr) - 1
    length = np.diff(rowptr).astype(np.int64)
    rows = np.repeat(np.arange(n), length)
    ord_ = np.argsort(length, kind="stable")
    plain = ord_.copy()
    for _ in range(2):
        inv = np.empty(n, dtype=np.int64)
        inv[ord_] = np.arange(n)
        first = first_ref(n, rows, col, inv)
        ord_ = ord_[np.argsort(length[ord_] * (n + 1) + first[ord_], kind="stable")]
    return plain, ord_, rows, length


def dead(n, rows, col, length, ord_):
    inv = np.empty(n, dtype=np.int64)
    inv[ord_] = np.arange(n)
    first = first_ref(n, rows, col, inv)
    nblk, npan = (n + 127) // 128, (n + 31) // 32
    fb = np.full(npan, nblk, dtype=np.int64)
    ref = first < n
    np.minimum.at(fb, inv[ref] // 32, first[ref] // 128)      # node at position inv[i], its first reader's block
    units = fb.sum() / (nblk * npan)
    # entries of block b cost one product per panel: the dead ones are those of the panels with first_block > b
    per_block = np.bincount(inv[rows] // 128, minlength=nblk).astype(np.float64)
    panels_dead_at = np.array([(fb > b).sum() for b in range(nblk)], dtype=np.float64)
    entries = (per_block * panels_dead_at).sum() / (per_block.sum() * npan)
    return units, entries


def main():
    names = sys.argv[1:] or ["pl32768d32", "pl32768", "pl65536", "er8192"]
    print(f"{'graph':12s} {'order':22s} {'units dead':>11s} {'entries in them':>16s}")
    for name in names:
        df = synth.WORKLOADS[name][0]()
        _, csr = ingest.directed(df, False, "from", "to", "weight")
        rowptr, col = np.asarray(csr.rowptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int64)
        plain, refined, rows, length = orders(rowptr, col)
        for label, o in (("length (stable)", plain), ("length, first (2 pass)", refined)):
            assert (np.diff(length[o]) >= 0).all()
            u, e = dead(len(length), rows, col, length, o)
            print(f"{name:12s} {label:22s} {100 * u:10.1f}% {100 * e:15.1f}%")


if __name__ == "__main__":
    main()
