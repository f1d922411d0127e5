"""libsimrank_profile.so (include/simrank_profile.h), ``count_pairs`` and ``threshold_for`` on a machine without a GPU:
header, binding and exports agree, the header is plain C99 and stands alone, the keys are order-preserving and
round-trip, ``simrank_profile_pick`` walks hand-made histograms, the host half of the radix select equals the NumPy
statement on emulated sweeps, a pruned model is answered from its lists, and every refusal comes before any device work."""
import math
import re
import struct

import numpy as np
import pytest

import simrank_amd.SimRank as SRA
from simrank_amd import _lib, _neighbors, _profile, _query
from tests import companion_abi as A
from tests import profile_ref as PR
from tests.host_doubles import HostOps, RingSpec, StubSpec, StubTables, boom


# ---- the library as a C library ------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    assert A.loaded_version(_profile) == _profile.VERSION == 1
    text = A.header(_profile)
    assert re.search(r"#define SIMRANK_PROFILE_MAX_EDGES %d\b" % _profile.MAX_EDGES, text) and _profile.MAX_EDGES == 1024
    assert re.search(r"#define SIMRANK_PROFILE_MAX_DIGIT_BITS %d\b" % _profile.MAX_DIGIT_BITS, text)
    A.assert_header_stands_alone(_profile)
    for bits, plan in _profile.DIGIT_PLAN.items():
        assert sum(plan) == bits and max(plan) <= _profile.MAX_DIGIT_BITS
    # the sweeps of threshold_for: at most 4 for f32, 2 for fp16-held, 8 for float64
    assert len(_profile.DIGIT_PLAN[32]) <= 4 and len(_profile.DIGIT_PLAN[16]) <= 2 and len(_profile.DIGIT_PLAN[64]) <= 8


def test_the_layout_codes_are_the_shared_ones():
    assert A.layout_codes(_profile) == A.layout_codes(_query)
    assert [_profile.key_bits(l) for l in range(4)] == [32, 32, 16, 64]
    assert _profile.load().simrank_profile_key_bits(4) == -1


def test_prototypes_match_the_header_argument_counts():
    A.assert_prototypes_match_the_header_argument_counts(_profile)


def test_companion_links_nothing_of_the_main_library():
    A.assert_links_nothing_of_the_main_library(_profile)


def test_the_main_library_is_unchanged():
    version, names, exports = A.main_library(_profile)
    assert version == _lib.ABI_VERSION == 8
    assert len(names) == 117 and len(exports) == 117


def test_header_is_c99_and_every_entry_refuses_bad_arguments_without_a_device(tmp_path):
    assert "profile 1 ok" in A.run_c99(_profile, tmp_path, r'''
#include <stdio.h>
#include <string.h>
#include "simrank_profile.h"
#define BAD(call, code) do { if ((call) != SIMRANK_PROFILE_ERR_INVALID) return code; \
                             if (!strlen(simrank_profile_last_error())) return 100 + code; } while (0)
int main(void) {
    float edges[2] = {0.0f, 1.0f};
    uint64_t counts[4] = {0, 0, 0, 0};
    uint64_t hist[4] = {5, 0, 3, 2};
    uint64_t above = 0;
    int32_t bin = 0;
    const int32_t f32 = SIMRANK_PROFILE_ROWMAJOR_F32;
    if (simrank_profile_version() != SIMRANK_PROFILE_VERSION) return 1;
    /* count: layout, NULL block, stride, panel alignment, n_edges, NULL edges / counts */
    BAD(simrank_profile_count(edges, 9, 4, 4, 4, NULL, NULL, edges, 2, counts, NULL), 2);
    BAD(simrank_profile_count(NULL, f32, 4, 4, 4, NULL, NULL, edges, 2, counts, NULL), 3);
    BAD(simrank_profile_count(edges, f32, 3, 4, 4, NULL, NULL, edges, 2, counts, NULL), 4);
    BAD(simrank_profile_count(edges, SIMRANK_PROFILE_PANEL_F16, 2, 4, 4, NULL, NULL, edges, 2, counts, NULL), 5);
    BAD(simrank_profile_count((const char*)counts + 4, SIMRANK_PROFILE_PANEL_F32, 4, 4, 4, NULL, NULL, edges, 2, counts, NULL), 6);
    BAD(simrank_profile_count(edges, f32, 4, 4, 4, NULL, NULL, edges, 0, counts, NULL), 7);
    BAD(simrank_profile_count(edges, f32, 4, 4, 4, NULL, NULL, edges, SIMRANK_PROFILE_MAX_EDGES + 1, counts, NULL), 8);
    BAD(simrank_profile_count(edges, f32, 4, 4, 4, NULL, NULL, NULL, 2, counts, NULL), 9);
    BAD(simrank_profile_count(edges, f32, 4, 4, 4, NULL, NULL, edges, 2, NULL, NULL), 10);
    BAD(simrank_profile_count(edges, f32, 2000000000, 2000000000, 2000000000, NULL, NULL, edges, 2, counts, NULL), 11);
    if (!strstr(simrank_profile_last_error(), "2^32")) return 12;
    if (simrank_profile_count(NULL, f32, 4, 0, 4, NULL, NULL, edges, 2, counts, NULL) != SIMRANK_PROFILE_OK) return 13;
    if (simrank_profile_count(NULL, f32, 4, 4, 0, NULL, NULL, edges, 2, counts, NULL) != SIMRANK_PROFILE_OK) return 14;
    /* digits: digit_bits, the key's width, a prefix wider than prefix_bits, NULL hist */
    BAD(simrank_profile_digits(edges, f32, 4, 4, 4, NULL, NULL, 0, 0, 0, hist, NULL, NULL), 20);
    BAD(simrank_profile_digits(edges, f32, 4, 4, 4, NULL, NULL, 0, 0, SIMRANK_PROFILE_MAX_DIGIT_BITS + 1, hist, NULL, NULL), 21);
    BAD(simrank_profile_digits(edges, f32, 4, 4, 4, NULL, NULL, 0, 24, 9, hist, NULL, NULL), 22);
    BAD(simrank_profile_digits(edges, SIMRANK_PROFILE_PANEL_F16, 4, 4, 4, NULL, NULL, 0, 8, 9, hist, NULL, NULL), 23);
    BAD(simrank_profile_digits(edges, f32, 4, 4, 4, NULL, NULL, 4, 2, 2, hist, NULL, NULL), 24);
    BAD(simrank_profile_digits(edges, f32, 4, 4, 4, NULL, NULL, 0, -1, 2, hist, NULL, NULL), 25);
    BAD(simrank_profile_digits(edges, f32, 4, 4, 4, NULL, NULL, 0, 0, 2, NULL, NULL, NULL), 26);
    BAD(simrank_profile_digits(edges, 7, 4, 4, 4, NULL, NULL, 0, 0, 2, hist, NULL, NULL), 27);
    if (simrank_profile_digits(NULL, f32, 4, 0, 4, NULL, NULL, 0, 0, 2, hist, NULL, NULL) != SIMRANK_PROFILE_OK) return 28;
    if (simrank_profile_key_bits(5) != SIMRANK_PROFILE_ERR_INVALID) return 30;
    if (simrank_profile_key_bits(SIMRANK_PROFILE_PANEL_F16) != 16) return 31;
    /* the host helpers */
    if (simrank_profile_key_f32(-0.0f) != simrank_profile_key_f32(0.0f)) return 40;
    if (simrank_profile_unkey_f64(simrank_profile_key_f64(-1.5)) != -1.5) return 41;
    if (simrank_profile_unkey_f16(simrank_profile_key_f16(0x3c00)) != 1.0 / 16384.0) return 42;
    BAD(simrank_profile_pick(NULL, 4, 0, 1, &bin, &above), 43);
    BAD(simrank_profile_pick(hist, 0, 0, 1, &bin, &above), 44);
    if (simrank_profile_pick(hist, 4, 0, 5, &bin, &above) != 1 || bin != 0 || above != 5) return 45;
    printf("profile %d ok\n", simrank_profile_version());
    return 0;
}
''')


# ---- keys -------------------------------------------------------------------------------------------------------------------
def _neighbours32(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def test_the_f32_key_is_monotone_and_round_trips():
    lib = _profile.load()
    f = np.float32
    tiny, big = f(np.finfo(f).tiny), f(np.finfo(f).max)
    denorm = f(1e-45)                                         # the smallest subnormal
    vals = [f(-np.inf), -big, f(-1.0), -tiny, -denorm, f(0.0), denorm, tiny, f(1.0), big, f(np.inf)]
    for x in (-1.0, 1.0, 0.5, 3.0e-39, -3.0e-39, 1.0e20):
        vals += _neighbours32(x)
    vals += [f(v) for v in np.random.default_rng(0).normal(size=200) * 10.0 ** np.random.default_rng(1).uniform(-40, 38, size=200)]
    vals = sorted(set(float(v) for v in vals))                # distinct values (0.0 once), ascending
    keys = [lib.simrank_profile_key_f32(v) for v in vals]
    assert all(a < b for a, b in zip(keys, keys[1:]))         # strictly monotone
    for v, k in zip(vals, keys):
        back = lib.simrank_profile_unkey_f32(k)
        assert struct.pack("<f", back) == struct.pack("<f", v)
    assert lib.simrank_profile_key_f32(-0.0) == lib.simrank_profile_key_f32(0.0) == 0x80000000
    assert not np.signbit(lib.simrank_profile_unkey_f32(lib.simrank_profile_key_f32(-0.0)))


def test_the_f64_key_is_monotone_and_round_trips():
    lib = _profile.load()
    tiny, big, denorm = np.finfo(np.float64).tiny, np.finfo(np.float64).max, 5e-324
    vals = [-np.inf, -big, -1.0, -tiny, -denorm, 0.0, denorm, tiny, 1.0, big, np.inf]
    for x in (-1.0, 1.0, 0.5, 1e-310, -1e-310, 1e200, float(np.float32(0.1))):
        vals += [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]
    vals += list(np.random.default_rng(2).normal(size=200) * 10.0 ** np.random.default_rng(3).uniform(-300, 300, size=200))
    vals = sorted(set(float(v) for v in vals))
    keys = [lib.simrank_profile_key_f64(v) for v in vals]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    for v, k in zip(vals, keys):
        assert struct.pack("<d", lib.simrank_profile_unkey_f64(k)) == struct.pack("<d", v)
    assert lib.simrank_profile_key_f64(-0.0) == lib.simrank_profile_key_f64(0.0) == 1 << 63
    assert not np.signbit(lib.simrank_profile_unkey_f64(lib.simrank_profile_key_f64(-0.0)))


def test_the_f16_key_orders_every_stored_value():
    """All 2^16 bit patterns but the NaNs: the key's order is the order of (float)h * 2^-14, and the inverse gives that value."""
    lib = _profile.load()
    bits = np.arange(1 << 16, dtype=np.uint16)
    h = bits.view(np.float16)
    ok = ~np.isnan(h)
    with np.errstate(invalid="ignore"):
        value = (h.astype(np.float32) * np.float32(2.0 ** -14)).astype(np.float64)
    keys = np.array([lib.simrank_profile_key_f16(int(b)) for b in bits], dtype=np.int64)
    assert keys.max() < 1 << 16
    order = np.argsort(keys[ok], kind="stable")
    v, k = value[ok][order], keys[ok][order]
    same = k[1:] == k[:-1]
    assert same.sum() == 1 and (v[1:][same] == 0).all()      # only -0.0 and +0.0 share a key
    assert (v[1:][~same] > v[:-1][~same]).all()
    for b in (0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x0400, 0x3c00, 0xbc00, 0x7bff, 0xfbff, 0x7c00, 0xfc00):
        back = lib.simrank_profile_unkey_f16(lib.simrank_profile_key_f16(b))
        assert back == value[b] and not (b == 0x8000 and np.signbit(back))


def test_edges_f32_is_the_smallest_float_at_or_above():
    ts = np.array([0.1, -0.1, 0.5, 1e-50, -1e-50, 0.0, -0.0, 1e39, -1e39, 1 + 2.0 ** -30, float(np.float32(0.3))])
    e = _profile.edges_f32(ts)
    assert e.dtype == np.float32
    assert (e.astype(np.float64) >= ts).all()
    with np.errstate(over="ignore"):
        below = np.nextafter(e, np.float32(-np.inf)).astype(np.float64)
    assert (below < ts).all()
    assert e[7] == np.inf and e[8] == -np.finfo(np.float32).max and e[3] == np.float32(1e-45) and e[4] == 0


# ---- pick and the host half of the select --------------------------------------------------------------------------------
def test_pick_on_hand_made_histograms():
    big = 2 ** 32 + 7
    # a bin count above 2^32, carried in 64 bits: the walk passes it and stops in the bin below
    assert _profile.pick([1, 9, big, 2], 3, big + 10) == (True, 1, big + 5)
    assert _profile.pick([1, 9, big, 2], 0, big + 11) == (True, 0, big + 11)
    assert _profile.pick([1, 9, big, 2], 0, 2 ** 63) == (False, 0, big + 11)      # everything fits: the lowest bin
    # a tie bin that straddles max_pairs: 4 above, the bin of 6 holds the 5th .. 10th
    for m in (4, 5, 9):
        assert _profile.pick([0, 7, 6, 0, 3, 1], 0, m) == (True, 2, 4)
    assert _profile.pick([0, 7, 6, 0, 3, 1], 0, 10) == (True, 1, 10)
    assert _profile.pick([0, 7, 6, 0, 3, 1], 0, 3) == (True, 4, 1)
    # the top bin alone is already too large: nothing above it, which ends as (inf, 0)
    assert _profile.pick([5, 0, 0, 8], 0, 7) == (True, 3, 0)
    assert _profile.pick([0, 0, 0, 0], 6, 7) == (False, -1, 6)
    assert _profile.pick([0, 2, 0, 0], 6, 7) == (True, 1, 6)
    assert _profile.pick([0, 2, 0, 0], 2 ** 64 - 2, 2 ** 64 - 1) == (True, 1, 2 ** 64 - 2)   # (no wrap-around)


def emulated_sweep(keys, bits):
    """What ``simrank_profile_digits`` computes, on a host array of keys (Python ints)."""
    keys = [int(k) for k in keys]

    def sweep(prefix, pbits, d, want_min):
        hist = np.zeros(1 << d, dtype=np.uint64)
        low = 2 ** 64 - 1
        for k in keys:
            head = k >> (bits - pbits) if pbits else 0
            if head == prefix:
                hist[(k >> (bits - pbits - d)) & ((1 << d) - 1)] += 1
            elif head > prefix:
                low = min(low, k)
        return hist, (low if want_min else None)
    return sweep


def hand_matrix():
    """4 x 4 with ties, -0.0, a NaN and negative values (the diagonal is no pair)."""
    return np.array([[9.0, 0.5, 0.5, -0.0],
                     [0.5, 9.0, 0.0, np.nan],
                     [-1.5, 0.25, 9.0, 0.0],
                     [-1.5, 0.25, 0.5, 9.0]])


def test_profile_ref_on_a_hand_made_matrix():
    S = hand_matrix()
    # off the diagonal: 0.5 x4, 0.25 x2, zeros x3 (one of them -0.0), -1.5 x2, one NaN
    ts = [0.5, 0.25, 0.0, -0.0, -1.5, -2.0, 0.6, 0.3, 1e-9, -1e-9]
    assert PR.count_pairs(S, ts).tolist() == [4, 6, 9, 9, 11, 11, 0, 4, 6, 9]
    want = {1: (math.inf, 0), 3: (math.inf, 0), 4: (0.5, 4), 5: (0.5, 4), 6: (0.25, 6), 8: (0.25, 6), 9: (0.0, 9), 10: (0.0, 9),
            11: (-1.5, 11), 12: (-1.5, 11), 100: (-1.5, 11)}
    for m, (t, n) in want.items():
        got = PR.threshold_for(S, m)
        assert got == (t, n) and not (t == 0 and np.signbit(got[0])), (m, got)
    assert PR.threshold_for(np.array([[1.0]]), 5) == (math.inf, 0)                 # no pair at all
    assert PR.threshold_for(np.array([[1.0, np.nan], [np.nan, 1.0]]), 5) == (math.inf, 0)
    # a mask that is not the diagonal: a block of a sharded iterate
    skip = np.zeros((4, 4), dtype=bool)
    skip[0, 1] = skip[3, 2] = True
    assert PR.count_pairs(S, [0.5, 9.0], skip).tolist() == [6, 4]


@pytest.mark.parametrize("bits", [32, 16, 64])
def test_the_host_half_of_the_select_equals_the_statement(bits):
    """``radix_select`` on emulated sweeps against ``profile_ref``, for every max_pairs, on the hand-made matrix and on
    matrices of distinct and of tie-heavy values (short digit plans too: the answer does not depend on the plan)."""
    lib = _profile.load()
    rng = np.random.default_rng(bits)
    mats = [hand_matrix(), rng.normal(size=(7, 7)).astype(np.float32).astype(np.float64),
            rng.choice([-0.0, 0.0, 2.0 ** -20, 0.25, 1.0], size=(6, 6)), np.full((3, 3), -0.0), np.array([[1.0]])]
    for S in mats:
        if bits == 16:                      # the values an fp16-held block holds: binary16 of value x 2^14, widened
            S = (np.clip(S, -3, 3) * 16384.0).astype(np.float16).astype(np.float64) / 16384.0
        v = PR.off_diagonal(S)
        v = v[~np.isnan(v)]
        if bits == 32:
            keys = [lib.simrank_profile_key_f32(float(x)) for x in v.astype(np.float32)]
        elif bits == 64:
            keys = [lib.simrank_profile_key_f64(float(x)) for x in v]
        else:
            keys = [lib.simrank_profile_key_f16(int(b)) for b in (v * 16384.0).astype(np.float16).view(np.uint16)]
        plans = [None, (8,) * (bits // 8), (5, 11) if bits == 16 else (1,) + (9,) * ((bits - 1) // 9) + ((bits - 1) % 9,) * (1 if (bits - 1) % 9 else 0)]
        for m in list(range(1, v.size + 3)) + [10 ** 12]:
            want = PR.threshold_for(S, m)
            for plan in plans:
                got = _profile.radix_select(emulated_sweep(keys, bits), bits, m, plan)
                assert got == want and not (got[0] == 0 and np.signbit(got[0])), (bits, m, plan, got, want)
            zeros = int((v == 0).sum())
            assert _profile.select_values(v[v != 0], zeros, m) == want


# ---- a pruned model: the host path ----------------------------------------------------------------------------------------
def test_a_pruned_model_is_answered_from_its_lists(monkeypatch):
    monkeypatch.setattr(_profile, "load", boom)                          # no library, no kernel
    ops = HostOps()
    n = 6
    ids = np.array([[3, 1, -1], [0, 2, 5], [-1, -1, -1], [5, 4, 0], [1, -1, -1], [2, 0, 4]], dtype=np.int32)
    vals = np.array([[0.5, 0.25, 0], [0.75, 0.75, 0.0], [0, 0, 0], [1.0, 0.5, 0.5], [-0.0, 0, 0], [0.125, 0.125, -1e-9]])
    solver = _neighbors.NeighborSolver(ops, [RingSpec(n)], [_neighbors.Tables.from_host(ops, ids, vals, np.ones(n))])
    est = SRA.SimRank()._keep(solver, [(0, list("abcdef"))])
    P = np.zeros((n, n))
    for a in range(n):
        P[a, ids[a][ids[a] >= 0]] = vals[a][ids[a] >= 0]
    P[np.arange(n), np.arange(n)] = 1.0
    ts = [0.5, 0.75, 0.1, 0.0, -0.0, -1e-9, -1.0, 2.0, 1e-12]
    got = est.count_pairs(ts)
    assert got.dtype == np.int64 and got.tolist() == PR.count_pairs(P, ts).tolist()
    assert got.tolist()[3] == n * (n - 1) - 1                            # the absent zeros count at t = 0
    for m in (1, 2, 3, 5, 6, 9, 28, 29, 30, 10 ** 9):
        assert est.threshold_for(m) == PR.threshold_for(P, m), m
    before = ops.live.copy()
    est.count_pairs([0.5])
    assert ops.live.keys() == before.keys()                              # the model is unchanged
    est.release()
    assert not ops.live


# ---- refusals: no device ---------------------------------------------------------------------------------------------------
def stubbed_estimator():
    """An estimator holding a solver whose device is never reached by what the argument checks do."""
    est = SRA.SimRank()
    solver = _neighbors.NeighborSolver(None, [StubSpec], [StubTables()])
    solver._make_reader = boom
    est._keep(solver, [(0, ["a", "b", "c"])])
    return est


def test_every_refusal_comes_before_any_device_work(monkeypatch):
    monkeypatch.setattr(_profile, "load", boom)
    monkeypatch.setattr(_profile, "count_pairs", boom)
    monkeypatch.setattr(_profile, "threshold_for", boom)
    monkeypatch.setattr(_profile, "count_blocks", boom)
    monkeypatch.setattr(_profile, "threshold_blocks", boom)
    est = stubbed_estimator()
    bad_thresholds = [[], (), [0.1] * 1025, [0.1, math.inf], [math.nan], [-math.inf], ["0.5"], [None], [True], 0.5, "0.5", None,
                      [0.1, [0.2]], np.array([0.1, np.inf]), [1 + 2j]]
    for bad in bad_thresholds:
        with pytest.raises(ValueError, match="threshold"):
            est.count_pairs(bad)
    for bad in (0, -1, 2.5, True, "3", None, math.inf, [5]):
        with pytest.raises(ValueError, match="max_pairs must be a positive integer"):
            est.threshold_for(bad)
    assert _profile.check_thresholds(np.array([0.5, -1, 0.5], dtype=np.float32)).tolist() == [0.5, -1.0, 0.5]
    assert _profile.check_thresholds([0.1] * 1024).size == 1024 and _profile.check_thresholds((1, np.int64(2))).tolist() == [1.0, 2.0]
    assert _profile.check_max_pairs(np.int64(7)) == 7 and _profile.check_max_pairs(2 ** 40) == 2 ** 40
    # no model, and a released one: the existing RuntimeErrors
    for call in (lambda e: e.count_pairs([0.5]), lambda e: e.threshold_for(10)):
        with pytest.raises(RuntimeError, match="no kept model"):
            call(SRA.SimRank())
    est.release()
    for call in (lambda e: e.count_pairs([0.5]), lambda e: e.threshold_for(10)):
        with pytest.raises(RuntimeError, match="released"):
            call(est)
