/*
 * simrank_cluster.h — single-linkage clusters of a similarity iterate that stays on the device (libsimrank_cluster.so).
 *
 * Which groups of nodes belong together at a threshold t: the connected components of the graph that joins two different
 * nodes a, b iff S[a][b] >= t or S[b][a] >= t.  The answer is one label per node; the matrix is swept IN PLACE, once for
 * up to SIMRANK_CLUSTER_MAX_LEVELS thresholds ("levels") together, and nothing but integers is ever written:
 *
 *     simrank_cluster_init     every node its own component in every level
 *     simrank_cluster_union    one block of the iterate: every entry that passes a level's threshold unites the two nodes
 *                              there.  The call ACCUMULATES: once per block (one block per rank's column range of a
 *                              sharded iterate), all into one parent array
 *     simrank_cluster_labels   the root of every node in every level
 *
 * The forest.  `parent` is device int32 [n_levels][n] over the node ids 0 .. n - 1 (the ids that row_ids / col_ids name).
 * At all times parent[x] <= x: a root is hooked only under a SMALLER root, with one integer compare-and-swap, so the root
 * a component ends with is its smallest id whatever the schedule was: the labels of two runs are the same integers.
 * Paths are shortened with ordinary stores of ancestors already read.  No thread ever waits for another: every walk to a
 * root and every retry of a hook carries an iteration cap of n + 8 (a chain cannot be longer), and a thread that reaches
 * it, or reads a parent above its node or outside 0 .. n - 1, ORs a bit into *status and gives up on that edge.  A caller
 * reads `status` with the labels: anything but 0 means the labels are not to be trusted (a parent array that was not
 * initialised, or overwritten).
 *
 * A block of n_rows x n_cols values is read as the plans of simrank_hip.h report it, in one of the four layouts below, as
 * simrank_profile.h reads it: row_ids / col_ids are device int32 (NULL = the positions 0, 1, ...); an id outside
 * 0 .. n - 1 is padding and its row or column is skipped, as are padding rows, padding columns, panel tails and the
 * entries with id(r) == id(c).  NaN passes no threshold; -0.0 >= +0.0 does.
 *
 * Conventions as simrank_profile.h: 0 or a negative status code (SIMRANK_CLUSTER_ERR_*), the message of the last failure
 * on the calling thread from simrank_cluster_last_error(); device pointers are HIP device memory of the current device;
 * `stream` is a hipStream_t passed as void*; the three entries only queue work on it and allocate nothing.  Argument
 * checks need no device.  Independent of the other headers of this project: this one includes none of them and the
 * library links none of their libraries.
 */
#ifndef SIMRANK_CLUSTER_H
#define SIMRANK_CLUSTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_CLUSTER_VERSION 1
#define SIMRANK_CLUSTER_MAX_LEVELS 8        /* thresholds of one sweep: they and a row's roots live in registers */

#if defined(__GNUC__)
#define SIMRANK_CLUSTER_API __attribute__((visibility("default")))
#else
#define SIMRANK_CLUSTER_API
#endif

enum {
    SIMRANK_CLUSTER_OK = 0,
    SIMRANK_CLUSTER_ERR_INVALID = -1,      /* bad argument: NULL, shape, layout, levels */
    SIMRANK_CLUSTER_ERR_HIP = -2           /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_CLUSTER_PANEL_F32 = 0,         /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_CLUSTER_ROWMAJOR_F32 = 1,      /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_CLUSTER_PANEL_F16 = 2,         /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_CLUSTER_ROWMAJOR_F64 = 3       /* float64 row-major: (r, c) at r * stride + c */
};

/* bits of *status (0 = every walk ended at a root) */
enum {
    SIMRANK_CLUSTER_BAD_PARENT = 1,        /* a parent above its node or outside 0 .. n - 1 was read */
    SIMRANK_CLUSTER_CAP_REACHED = 2        /* a walk or a retry loop reached its cap of n + 8 steps */
};

SIMRANK_CLUSTER_API int simrank_cluster_version(void);
SIMRANK_CLUSTER_API const char* simrank_cluster_last_error(void);

/* parent[l * n + i] = i for l < n_levels (1 .. SIMRANK_CLUSTER_MAX_LEVELS), i < n (0 <= n < 2^31); *status = 0.
 * `parent`: device int32 [n_levels][n]; `status`: one device int32.  Asynchronous on `stream`. */
SIMRANK_CLUSTER_API int simrank_cluster_init(int32_t* parent, int64_t n, int32_t n_levels, int32_t* status, void* stream);

/* Every entry v of the block with id(r) != id(c), both ids in 0 .. n - 1, unites id(r) and id(c) in every level l with
 * v >= edges[l]; with ascending edges, an entry >= the j lowest of them unites in levels 0 .. j - 1.  `edges`: device
 * array of n_levels thresholds in the type they are compared in: float for the f32 layouts and for binary16 (read as
 * (float)h * 2^-14, what the dense hand-back widens), double for float64.  `parent` and `status` as simrank_cluster_init
 * left them or as earlier calls of this entry did: the call adds its block's edges to them.  One sweep of the block for
 * all levels, 16-byte loads along the contiguous direction of the layout; per entry and level one read of the column
 * node's parent decides whether anything is left to do, a wave passes each distinct pair of roots on to the
 * compare-and-swap once, and integer atomics are the only atomics.  Asynchronous on `stream`. */
SIMRANK_CLUSTER_API int simrank_cluster_union(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                              const int32_t* row_ids, const int32_t* col_ids, const void* edges,
                                              int32_t n_levels, int32_t* parent, int64_t n, int32_t* status, void* stream);

/* labels[l * n + i] = the root of i in level l: once every block went through simrank_cluster_union, the smallest id of
 * i's component.  `labels`: device int32 [n_levels][n], not `parent` itself.  `parent` is only read.  Asynchronous on
 * `stream`. */
SIMRANK_CLUSTER_API int simrank_cluster_labels(const int32_t* parent, int64_t n, int32_t n_levels, int32_t* labels,
                                               int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_CLUSTER_H */
