/*
 * simrank_hdbscan.h — core similarities and the mutual-reachability picks of a similarity iterate that stays on the
 * device (libsimrank_hdbscan.so): the two device primitives of HDBSCAN* that simrank_linkage.h and simrank_density.h
 * lack.
 *
 * Two different nodes a, b have the PAIR HEIGHT w(a, b) = max(S[a][b], S[b][a]): simrank_linkage.h's.  A NaN entry is no
 * entry (one NaN: the other direction decides; two: the pair does not exist); -0.0 and +0.0 are one value, +0.0.  The
 * CORE SIMILARITY of a node a at a rank k >= 1 is the k-th largest of its existing w(a, b), b != a: +inf at k = 0 (the
 * node counts itself: k = min_samples - 1) and -inf when fewer than k pairs exist.  It is a selection, hence exact.  The
 * MUTUAL REACHABILITY of a pair is min(w(a, b), core(a), core(b)); -inf is no entry.  Single linkage on it is HDBSCAN*'s
 * hierarchy: simrank_hdbscan_pick is simrank_linkage_pick with the entries clamped that way, and simrank_linkage.h's
 * init, hook and flatten run around it unchanged.
 *
 * The symmetric select.  A multi-pass radix select, most significant digit first, on an order-preserving unsigned key
 * of w: 16 bits for binary16, 32 for f32, 64 for float64; the key 0 belongs to no value and stands for NaN, so the key
 * of w is the integer maximum of the two directions' keys, and both zeros share one key.  Per node the device keeps
 * the key prefix found so far (uint64), the remaining rank (int32; 0: +inf, -1: fewer pairs than the rank) and a
 * histogram of SIMRANK_HDBSCAN_BINS int32 counters:
 *
 *     simrank_hdbscan_select_init    prefix 0, the rank, the counters 0
 *     then, for pass = 0 .. simrank_hdbscan_select_passes(layout) - 1:
 *       simrank_hdbscan_select_count one sweep of the SQUARE block: hist[id(a)][d] += the positions b != a whose key
 *                                    agrees with a's prefix above this pass' digit and has the digit d
 *       simrank_hdbscan_select_step  per node: the bins walked from the top, the digit fixed, the rank lowered by the
 *                                    counts above it, the bins cleared
 *     simrank_hdbscan_select_finish  core as float64 [n] and in the block's compare type [n]
 *     (simrank_hdbscan_select queues all of these)
 *
 * The count sweep has the shape of simrank_density_degrees: one workgroup per pair of 64 x 64 tiles (I, J), I <= J; both
 * tiles go through LDS as keys (2 x 64 x 64 words: 32 KiB for the 32-bit keys of f32 and binary16, 64 KiB for float64),
 * column c of row r at word r * 64 + (c ^ r): a row and a column of a tile each touch 64 different words, so neither
 * the wave that stores a row nor the one that reads a column transposed meets a bank conflict, and no padding word is
 * needed (a padded row would take a float64 pair of tiles past the 64 KiB a workgroup may declare).  The wave that
 * holds row a of one tile reads v(b, a) transposed from the other and forms the key of w; per digit value present in
 * the row it counts the lanes whose key matches with one ballot and a popcount, never with an atomic per element: the
 * matrices are full of ties and exact zeros, and such atomics would all hit one counter.  A diagonal tile pairs with
 * itself and the position a itself is skipped.  Every element is read once per sweep, 64-bit offsets throughout;
 * integer atomic adds into the counters are the only atomics; every loop is bounded by a constant or by n and nothing
 * waits on another thread.
 *
 * The digit is SIMRANK_HDBSCAN_DIGIT_BITS = 4 bits wide: 4 sweeps of a binary16 block, 8 of an f32 and 16 of a float64
 * one.  Measured at N = 32768, a sweep takes 3.0 ms on f32 and 2.9 to 3.7 ms on binary16 whatever the
 * pass finds, 1.4 to 1.6 times an 8-level simrank_density_degrees sweep over the same bytes in the same shape: what it
 * costs is the walk itself (the loads, the keys through LDS, two LDS reads and a compare per row), not the counting,
 * so fewer and wider passes are what pays, up to what the counting can hold.  With 4 bits the 16 counts of a row live
 * in 16 lanes of the wave that owns it and a node's counters are ONE 64-byte line, which every atomic of a row falls
 * into: 64 bytes of state per node, no LDS beyond the tiles.  An 8-bit digit would halve the sweeps but needs 256
 * counts per row (four per lane, or LDS that the 64 KiB of a float64 pair of tiles leave no room for in a
 * workgroup's static 64 KiB) and 1 KiB of counters per node, 32 MiB at N = 32768, touched line by line; a 2-bit digit
 * doubles the sweeps of a matrix that no cache holds and saves nothing a sweep spends its time on.
 *
 * A block is read as the plans of simrank_hip.h report it, in one of the four layouts below; ids are device int32
 * (NULL = the positions 0, 1, ...) naming the nodes 0 .. n - 1; an id outside them is padding, and its row and column
 * are skipped, as are panel tails and the padding of a stride.
 *
 * Conventions as simrank_linkage.h: 0 or a negative status code (SIMRANK_HDBSCAN_ERR_*), the message of the last failure
 * on the calling thread from simrank_hdbscan_last_error(); device pointers are HIP device memory of the current device;
 * `stream` is a hipStream_t passed as void*; the entries only queue work on it and allocate nothing.  Argument checks
 * need no device.  Independent of the other headers of this project: this one includes none of them and the library
 * links none of their libraries.
 */
#ifndef SIMRANK_HDBSCAN_H
#define SIMRANK_HDBSCAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_HDBSCAN_VERSION 1
#define SIMRANK_HDBSCAN_TILE 64             /* a tile is 64 x 64 entries: a row is one wave */
#define SIMRANK_HDBSCAN_DIGIT_BITS 4        /* bits of the key fixed per pass of the select */
#define SIMRANK_HDBSCAN_BINS 16             /* 1 << SIMRANK_HDBSCAN_DIGIT_BITS counters per node */

#if defined(__GNUC__)
#define SIMRANK_HDBSCAN_API __attribute__((visibility("default")))
#else
#define SIMRANK_HDBSCAN_API
#endif

enum {
    SIMRANK_HDBSCAN_OK = 0,
    SIMRANK_HDBSCAN_ERR_INVALID = -1,      /* bad argument: NULL, shape, layout, pass, phase, rank */
    SIMRANK_HDBSCAN_ERR_HIP = -2           /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_HDBSCAN_PANEL_F32 = 0,         /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_HDBSCAN_ROWMAJOR_F32 = 1,      /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_HDBSCAN_PANEL_F16 = 2,         /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_HDBSCAN_ROWMAJOR_F64 = 3       /* float64 row-major: (r, c) at r * stride + c */
};

/* bits of *status of simrank_hdbscan_pick (0 = every read was in order): simrank_linkage.h's */
enum {
    SIMRANK_HDBSCAN_BAD_COMPONENT = 1      /* a component outside 0 .. n - 1 was read */
};

SIMRANK_HDBSCAN_API int simrank_hdbscan_version(void);
SIMRANK_HDBSCAN_API const char* simrank_hdbscan_last_error(void);

/* The count sweeps a select of `layout` takes: key bits / SIMRANK_HDBSCAN_DIGIT_BITS = 8 (f32), 4 (binary16) or 16
 * (float64); SIMRANK_HDBSCAN_ERR_INVALID for an unknown layout. */
SIMRANK_HDBSCAN_API int simrank_hdbscan_select_passes(int32_t layout);

/* prefix[i] = 0, remaining[i] = min(rank, 2^31 - 1), hist[i][d] = 0 for i < n (0 <= n < 2^31 - 8), d <
 * SIMRANK_HDBSCAN_BINS.  `rank` >= 0: the core similarity wanted is the rank-th largest pair height of every node
 * (min_samples - 1).  `prefix`: device uint64 [n]; `remaining`: device int32 [n]; `hist`: device int32 [n][BINS].
 * Asynchronous on `stream`. */
SIMRANK_HDBSCAN_API int simrank_hdbscan_select_init(uint64_t* prefix, int32_t* remaining, int32_t* hist, int64_t n,
                                                    int64_t rank, void* stream);

/* One count sweep, pass `pass` (0 .. passes - 1, the most significant digit first), of the SQUARE block S of n x n
 * values, position p being the node ids[p] (NULL: p itself): for every position a whose id is a node, and every
 * position b != a whose id is a node and whose key k of w(a, b) is not 0 (the pair exists) and agrees with
 * prefix[id(a)] in the digits of the earlier passes, hist[id(a)][digit `pass` of k] += 1.  `prefix` is only read.
 * Asynchronous on `stream`. */
SIMRANK_HDBSCAN_API int simrank_hdbscan_select_count(const void* S, int32_t layout, int64_t stride, int64_t n,
                                                     const int32_t* ids, int32_t pass, const uint64_t* prefix,
                                                     int32_t* hist, void* stream);

/* Per node i with remaining[i] > 0: the bins from the top down, d the first digit with remaining[i] <= the count of d
 * and the digits above it; prefix[i] gets d as its digit `pass` and remaining[i] loses the counts above d; when the
 * bins hold fewer than remaining[i] in all, remaining[i] = -1.  hist[i][*] = 0 for every node.  Asynchronous on
 * `stream`. */
SIMRANK_HDBSCAN_API int simrank_hdbscan_select_step(int32_t layout, int32_t pass, uint64_t* prefix, int32_t* remaining,
                                                    int32_t* hist, int64_t n, void* stream);

/* core[i] = +inf where remaining[i] == 0, -inf where it is negative, else the value whose key is prefix[i] (+0.0 for the
 * zeros; a binary16 key widened as the dense hand-back widens it): written twice, as double into core64 [n] and in the
 * block's compare type into core_cmp [n] (float for the f32 layouts and binary16, double for float64; the narrowing is
 * exact: the values are stored values or infinities).  Either may be NULL.  Asynchronous on `stream`. */
SIMRANK_HDBSCAN_API int simrank_hdbscan_select_finish(int32_t layout, const uint64_t* prefix, const int32_t* remaining,
                                                      int64_t n, double* core64, void* core_cmp, void* stream);

/* All of the above in order: init, passes x (count, step), finish.  1 + 2 passes + 1 launches. */
SIMRANK_HDBSCAN_API int simrank_hdbscan_select(const void* S, int32_t layout, int64_t stride, int64_t n, const int32_t* ids,
                                               int64_t rank, uint64_t* prefix, int32_t* remaining, int32_t* hist,
                                               double* core64, void* core_cmp, void* stream);

/* simrank_linkage_pick with one more argument.  `core`: device [n] in the compare type, indexed by node id, only read.
 * The candidate value of entry (r, c) is min(v, core[id(r)], core[id(c)]); NaN and -inf are no candidates; the floor
 * applies to the clamped value.  Everything else is simrank_linkage_pick's: the `best` slot format (so that
 * simrank_linkage_hook and _flatten take the slots as they are), phases 0 and 1 of a float64 block, the slot read before
 * every atomic, 64-bit integer maxima the only atomics, one launch per call that must stay a kernel of its own.  Each
 * direction of a pair is a candidate of its own, and the larger of the two clamped entries is the mutual reachability:
 * no pairing is needed here.  Asynchronous on `stream`. */
SIMRANK_HDBSCAN_API int simrank_hdbscan_pick(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                             const int32_t* row_ids, const int32_t* col_ids, const void* floor, int32_t phase,
                                             const void* core, const int32_t* comp, uint64_t* best, int64_t n,
                                             int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_HDBSCAN_H */
