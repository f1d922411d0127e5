/*
 * simrank_profile.h — the distribution of a similarity iterate that stays on the device (libsimrank_profile.so).
 *
 * Two global questions about a kept model, answered by sweeps of the iterate IN PLACE, exact in integers:
 *
 *     simrank_profile_count    how many off-diagonal entries lie in each interval between sorted thresholds
 *                              (the host turns intervals into ">= t" counts with a suffix sum)
 *     simrank_profile_digits   one pass of a GLOBAL radix select on an order-preserving integer key of the stored value:
 *                              among the entries whose key starts with `prefix`, a histogram of the next digit
 *
 * Both read a block of n_rows x n_cols values as the plans of simrank_hip.h report it (simrank_plan_get & co: "iterate",
 * "iterate_layout", "iterate_stride", "iterate_rows", "iterate_col_lo", "iterate_col_hi", "ids") in one of the four
 * layouts below, and both ADD to the counters they are given: the caller zeroes them once and calls once per block (one
 * block per rank's column range of a sharded iterate).  An entry (r, c) is skipped where id(r) == id(c) (row_ids /
 * col_ids: device int32; NULL = the positions 0, 1, ...).  Padding rows, padding columns and panel tails are never
 * counted.  Counters are 64-bit: a block of 65536 x 65536 holds more than 2^32 entries.
 *
 * The key: f32 and float64 values map to unsigned integers of their width whose order is the values' order; -0.0 and +0.0
 * share one key (+0.0's); NaN has no place in the order and is never counted.  A binary16 held as value x 2^14 has a
 * 16-bit key of its own bits (the scale is a power of two: the order is the same).
 *
 * The host helpers (keys, their inverses, simrank_profile_pick) touch no device.
 *
 * A measuring switch, to be removed: before its local-memory atomics a sweep takes the dominant bins of a wave out of the
 * way with two ballot rounds (profile.hip).  While the environment variable SIMRANK_PROFILE_PLAIN is set to anything but
 * "" or "0" (read at every call of the two sweeps), the same kernels run WITHOUT those rounds; the results are the same
 * counts.  It exists only so that tools/bench_profile.py can time both forms in one run; once that has decided, the
 * slower form, its kernel instantiations and this variable go.  Nothing else reads the environment.
 *
 * Conventions as simrank_select.h: 0 or a negative status (SIMRANK_PROFILE_ERR_*), the message of the last failure on the
 * calling thread from simrank_profile_last_error(); device pointers are HIP device memory of the current device; `stream`
 * is a hipStream_t passed as void*; the two sweeps only queue work on it and allocate nothing.  Argument checks need no
 * device.  Independent of the other headers of this project: this one includes none of them and the library links none
 * of their libraries.
 */
#ifndef SIMRANK_PROFILE_H
#define SIMRANK_PROFILE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_PROFILE_VERSION 1
#define SIMRANK_PROFILE_MAX_EDGES 1024      /* thresholds of one count sweep: they and their bins live in local memory */
#define SIMRANK_PROFILE_MAX_DIGIT_BITS 11   /* 2048 bins of a digit sweep in local memory */

#if defined(__GNUC__)
#define SIMRANK_PROFILE_API __attribute__((visibility("default")))
#else
#define SIMRANK_PROFILE_API
#endif

enum {
    SIMRANK_PROFILE_OK = 0,
    SIMRANK_PROFILE_ERR_INVALID = -1,      /* bad argument: NULL, shape, layout, edges, digits */
    SIMRANK_PROFILE_ERR_HIP = -2           /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_PROFILE_PANEL_F32 = 0,         /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_PROFILE_ROWMAJOR_F32 = 1,      /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_PROFILE_PANEL_F16 = 2,         /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_PROFILE_ROWMAJOR_F64 = 3       /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_PROFILE_API int simrank_profile_version(void);
SIMRANK_PROFILE_API const char* simrank_profile_last_error(void);

/* Bits of the key of a layout's values: 32 (f32), 16 (binary16), 64 (float64); SIMRANK_PROFILE_ERR_INVALID otherwise. */
SIMRANK_PROFILE_API int simrank_profile_key_bits(int32_t layout);

/* counts[j] += the number of entries v of the block (id(r) != id(c)) with exactly j of the edges <= v, j = 0 .. n_edges.
 * `edges`: device array of n_edges (1 .. SIMRANK_PROFILE_MAX_EDGES) thresholds sorted ascending, in the type they are
 * compared in: float for the f32 layouts and for binary16 (read as (float)h * 2^-14, what the dense hand-back widens),
 * double for float64.  `counts`: device uint64 [n_edges + 1].  NaN compares false and lands in counts[0]; -0.0 >= +0.0.
 * The entries >= edges[i] are counts[i + 1] + ... + counts[n_edges].  16-byte loads along the contiguous direction of
 * the layout; a workgroup counts in 32-bit bins of local memory (a call whose workgroups would each see 2^32 entries is
 * refused) and adds them to `counts` once, with 64-bit atomic adds.  Asynchronous on `stream`. */
SIMRANK_PROFILE_API int simrank_profile_count(const void* S, int32_t layout, int64_t stride, int64_t n_rows,
                                              int64_t n_cols, const int32_t* row_ids, const int32_t* col_ids,
                                              const void* edges, int32_t n_edges, uint64_t* counts, void* stream);

/* One pass of the radix select.  With B = simrank_profile_key_bits(layout): among the entries (id(r) != id(c), not NaN)
 * whose key's top `prefix_bits` bits equal `prefix`,
 *     hist[(key >> (B - prefix_bits - digit_bits)) & (2^digit_bits - 1)] += 1        device uint64 [2^digit_bits]
 * and, when `min_above` (device uint64, one element) is not NULL, *min_above = min(*min_above, key) over the entries
 * whose top prefix_bits bits are GREATER than `prefix` (start it at UINT64_MAX).  0 <= prefix_bits, 1 <= digit_bits <=
 * SIMRANK_PROFILE_MAX_DIGIT_BITS, prefix_bits + digit_bits <= B, prefix < 2^prefix_bits.  Asynchronous on `stream`. */
SIMRANK_PROFILE_API int simrank_profile_digits(const void* S, int32_t layout, int64_t stride, int64_t n_rows,
                                               int64_t n_cols, const int32_t* row_ids, const int32_t* col_ids,
                                               uint64_t prefix, int32_t prefix_bits, int32_t digit_bits, uint64_t* hist,
                                               uint64_t* min_above, void* stream);

/* Host only: the keys and their inverses.  a < b  <=>  key(a) < key(b) for values that are not NaN; key(-0.0) ==
 * key(+0.0) and the inverse gives +0.0.  The binary16 pair takes the stored bits and gives back the VALUE the block
 * means: (double)((float)h * 2^-14). */
SIMRANK_PROFILE_API uint32_t simrank_profile_key_f32(float v);
SIMRANK_PROFILE_API float simrank_profile_unkey_f32(uint32_t key);
SIMRANK_PROFILE_API uint64_t simrank_profile_key_f64(double v);
SIMRANK_PROFILE_API double simrank_profile_unkey_f64(uint64_t key);
SIMRANK_PROFILE_API uint32_t simrank_profile_key_f16(uint16_t half_bits);
SIMRANK_PROFILE_API double simrank_profile_unkey_f16(uint32_t key);

/* Host only: which bin the select descends into.  `hist` [bins] is a digit histogram under the current prefix and
 * `above` the number of entries whose key lies above every key of that prefix.  Walking from the top bin down while
 * above + (the bins walked) <= max_pairs:
 *     a bin that no longer fits      *bin = that bin, *above_out = above + the bins over it; returns 1
 *     every bin fits, some entry     *bin = the lowest bin that is not empty, *above_out = above + the bins over it;
 *                                    returns 0
 *     no entry at all                *bin = -1, *above_out = above; returns 0
 * At the last digit the bin is a key k: the answer is k itself when above_out + hist[bin] <= max_pairs, otherwise the
 * next larger key that occurs, with above_out entries (none: nothing fits). */
SIMRANK_PROFILE_API int simrank_profile_pick(const uint64_t* hist, int32_t bins, uint64_t above, uint64_t max_pairs,
                                             int32_t* bin, uint64_t* above_out);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_PROFILE_H */
