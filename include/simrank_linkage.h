/*
 * simrank_linkage.h — the single-linkage dendrogram of a similarity iterate that stays on the device
 * (libsimrank_linkage.so).
 *
 * The dendrogram of "two different nodes a, b are joined at height w(a, b) = max(S[a][b], S[b][a])" is a maximum spanning
 * forest of that graph: n - 1 edges or fewer, of which every threshold's components (simrank_cluster.h) are a cut.
 * Boruvka's algorithm finds one in at most ceil(log2 n) rounds, each one sweep of the matrix IN PLACE; nothing but
 * integers and the n records of the forest is ever written:
 *
 *     simrank_linkage_init      every node its own component, no record, *status = *n_hooked = 0
 *     then, until a round hooks nothing (the host reads *n_hooked and *status after each):
 *       simrank_linkage_pick    one block of the iterate: every component's best entry towards another component.  The call
 *                               ACCUMULATES: once per block (one block per rank's column range of a sharded iterate), all
 *                               into one array of slots.  A float64 iterate takes the calls of every block with phase 0,
 *                               then again with phase 1
 *       simrank_linkage_hook    every component with a pick goes under the component it picked and records the edge
 *       simrank_linkage_flatten every node learns its new component; the slots are emptied
 *
 * Components.  `comp` is device int32 [n] over the node ids 0 .. n - 1 (the ids that row_ids / col_ids name): between
 * rounds comp[x] is the root of x's component, a node with comp[r] == r.
 *
 * Picks.  An entry v at (r, c) with comp[id(r)] != comp[id(c)], v not NaN and v >= *floor (when a floor is given) is a
 * candidate of BOTH components.  A component keeps the candidate with the largest value and, among equal values, the
 * smallest root on the other side; -0.0 and +0.0 are one value.  This is one strict order on the unordered pairs of roots
 * that all components share, so the picks of a round form no cycle but the mutual pick of two components.  `best` is
 * device uint64 [2][n], indexed by root.  The f32 and binary16 layouts use best[0] alone: an order-preserving 32-bit key of
 * the value in the high half, 0xffffffff - other root in the low half, under one 64-bit integer maximum; 0 = no pick.  A
 * float64 key fills a word: phase 0 keeps the largest key in best[0], phase 1 the largest 0xffffffff - other root among
 * the entries whose key is the one in best[0] in best[1].
 *
 * Hooks.  Of a mutual pick the smaller root stays and the larger goes under it; every other pick goes under its target.
 * A root is hooked at most once in its life, so the edge lives at its own index: hook_other[c] (device int32 [n], -1 =
 * never hooked) is the root c went under and hook_value[c] (device double [n]) the value of the pick, widened as the dense
 * hand-back widens it, +0.0 for either zero.  The records with hook_other[c] >= 0 are the forest: between the two ROOTS,
 * which need not be the entry's own nodes, at the largest value between the two components.  Every threshold cuts this
 * forest into the components the matrix has there.  Which forest it is does not depend on the schedule.
 *
 * One launch per call.  A pick reads `comp`, and in phase 1 the keys in best[0], through the compute unit's caches,
 * as earlier calls left them: every entry is a kernel of its own on `stream`, in the order above, and what is right
 * about it rests on the cache invalidate at the start of a kernel.  A port that fuses a pick with init, hook, flatten
 * or the pick of the other phase, or replays them without that acquire, has to read those words at device scope.
 *
 * No thread ever waits for another.  A walk to a root carries a cap of n + 8 steps; a walk that reaches it, or any read of
 * a component or a pick outside 0 .. n - 1, ORs a bit into *status and stops: anything but 0 means the records are not to
 * be trusted (arrays that were not initialised, or overwritten).
 *
 * A block of n_rows x n_cols values is read as simrank_cluster.h reads it, in one of the four layouts below: row_ids /
 * col_ids are device int32 (NULL = the positions 0, 1, ...); an id outside 0 .. n - 1 is padding and its row or column is
 * skipped, as are padding rows, padding columns, panel tails and the entries with id(r) == id(c).
 *
 * Conventions as simrank_cluster.h: 0 or a negative status code (SIMRANK_LINKAGE_ERR_*), the message of the last failure
 * on the calling thread from simrank_linkage_last_error(); device pointers are HIP device memory of the current device;
 * `stream` is a hipStream_t passed as void*; the four entries only queue work on it and allocate nothing.  Argument
 * checks need no device.  Independent of the other headers of this project: this one includes none of them and the
 * library links none of their libraries.
 */
#ifndef SIMRANK_LINKAGE_H
#define SIMRANK_LINKAGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_LINKAGE_VERSION 1

#if defined(__GNUC__)
#define SIMRANK_LINKAGE_API __attribute__((visibility("default")))
#else
#define SIMRANK_LINKAGE_API
#endif

enum {
    SIMRANK_LINKAGE_OK = 0,
    SIMRANK_LINKAGE_ERR_INVALID = -1,      /* bad argument: NULL, shape, layout, phase */
    SIMRANK_LINKAGE_ERR_HIP = -2           /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_LINKAGE_PANEL_F32 = 0,         /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_LINKAGE_ROWMAJOR_F32 = 1,      /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_LINKAGE_PANEL_F16 = 2,         /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_LINKAGE_ROWMAJOR_F64 = 3       /* float64 row-major: (r, c) at r * stride + c */
};

/* bits of *status (0 = every read was in order) */
enum {
    SIMRANK_LINKAGE_BAD_COMPONENT = 1,     /* a component or a picked root outside 0 .. n - 1 was read */
    SIMRANK_LINKAGE_CAP_REACHED = 2        /* a walk to a root reached its cap of n + 8 steps */
};

SIMRANK_LINKAGE_API int simrank_linkage_version(void);
SIMRANK_LINKAGE_API const char* simrank_linkage_last_error(void);

/* The picks of `layout` need phase 0 alone (1), or phase 0 over every block and then phase 1 over every block (2);
 * SIMRANK_LINKAGE_ERR_INVALID for an unknown layout. */
SIMRANK_LINKAGE_API int simrank_linkage_phases(int32_t layout);

/* comp[i] = i, best[0][i] = best[1][i] = 0, hook_other[i] = -1, hook_value[i] = 0 for i < n (0 <= n < 2^31 - 8);
 * *status = *n_hooked = 0.  `status`, `n_hooked`: one device int32 each.  Asynchronous on `stream`. */
SIMRANK_LINKAGE_API int simrank_linkage_init(int32_t* comp, uint64_t* best, int32_t* hook_other, double* hook_value, int64_t n,
                                             int32_t* n_hooked, int32_t* status, void* stream);

/* One sweep of the block: its candidates go into `best` as described above.  `floor`: NULL, or a HOST pointer to one
 * value in the type entries are compared in, read before the call returns: float for the f32 layouts and for binary16
 * (read as (float)h * 2^-14, what the dense hand-back widens), double for float64; an entry below it is no candidate.
 * `phase`: 0, or 1 for the second sweep of a float64 block.  `comp` is only read.  16-byte loads along the contiguous
 * direction of the layout; the row's side is reduced in registers and across the lanes of the row and costs one atomic
 * per row, the column's side reads its slot first and issues the atomic only for a candidate that beats what it read (a
 * slot only grows within a round, so a stale read costs an atomic and never a pick).  64-bit integer maxima are the only
 * atomics.  Asynchronous on `stream`. */
SIMRANK_LINKAGE_API int simrank_linkage_pick(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                             const int32_t* row_ids, const int32_t* col_ids, const void* floor, int32_t phase,
                                             const int32_t* comp, uint64_t* best, int64_t n, int32_t* status, void* stream);

/* Every root c with a pick: unless the pick is mutual and c the smaller root, comp[c] = hook_other[c] = the picked root,
 * hook_value[c] = the picked value, and *n_hooked grows by one (it counts since simrank_linkage_init).  `key_bits`: 32
 * for picks of the f32 and binary16 layouts, 64 for float64.  `best` is only read.  Asynchronous on `stream`. */
SIMRANK_LINKAGE_API int simrank_linkage_hook(const uint64_t* best, int32_t key_bits, int32_t* comp, int32_t* hook_other,
                                             double* hook_value, int64_t n, int32_t* n_hooked, int32_t* status, void* stream);

/* comp[i] = the root above i, best[0][i] = best[1][i] = 0.  Asynchronous on `stream`. */
SIMRANK_LINKAGE_API int simrank_linkage_flatten(int32_t* comp, uint64_t* best, int64_t n, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_LINKAGE_H */
