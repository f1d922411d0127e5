/*
 * simrank_density.h — density clusters (DBSCAN) of a similarity iterate that stays on the device (libsimrank_density.so).
 *
 * Two different nodes a, b are NEIGHBOURS at a threshold t iff S[a][b] >= t or S[b][a] >= t: the relation of
 * simrank_cluster.h.  A pair that passes in both directions is one neighbour.  The library counts every node's
 * neighbours, and grows clusters through the nodes that have enough of them:
 *
 *     simrank_density_init      counters 0, every node its own root, no node attached, *status = 0
 *     simrank_density_degrees   deg[l][id(a)] += the number of positions b != a with v(a, b) >= edges[l] or
 *                               v(b, a) >= edges[l], for up to SIMRANK_DENSITY_MAX_LEVELS thresholds in ONE sweep of a
 *                               square block that reads every element once: entry (a, b) meets entry (b, a) in the
 *                               workgroup that holds both of their 64 x 64 tiles
 *     simrank_density_union     one level, one block of the iterate; a node x is a CORE node iff deg[x] >= min_neighbors.
 *                               Every entry between two different nodes that passes `edge`: both core -> the two are
 *                               united; exactly one core -> attach[the other] = min(attach[the other], the core node);
 *                               neither -> nothing.  The call ACCUMULATES: once per block, all into one forest
 *     simrank_density_labels    a core node's root; a border node's (not core, attached) root of the node it is attached
 *                               to; -1 for noise (not core, not attached)
 *
 * Everything written is an integer and every sum, minimum and root is independent of the schedule: counts are added with
 * integer atomics, `attach` only falls (an atomic minimum: a border node ends at its SMALLEST core neighbour), and the
 * forest is simrank_cluster.h's: parent[x] <= x at all times, a root is hooked only under a smaller root with one
 * compare-and-swap, so a cluster's root is its smallest core node.  No thread ever waits for another: every walk to a
 * root and every retry of a hook carries a cap of n + 8 steps, and a thread that reaches it, or reads a parent or an
 * attachment out of order, ORs a bit into *status and gives up on that edge.  Anything but 0 there means the labels are
 * not to be trusted.
 *
 * A block is read as the plans of simrank_hip.h report it, in one of the four layouts below; ids are device int32
 * (NULL = the positions 0, 1, ...) naming the nodes 0 .. n - 1; an id outside them is padding, and its row and column
 * are skipped, as are panel tails and the padding of a stride.  NaN passes no threshold; -0.0 >= +0.0 does.
 *
 * Conventions as simrank_cluster.h: 0 or a negative status code (SIMRANK_DENSITY_ERR_*), the message of the last failure
 * on the calling thread from simrank_density_last_error(); device pointers are HIP device memory of the current device;
 * `stream` is a hipStream_t passed as void*; the four entries only queue work on it and allocate nothing.  Argument
 * checks need no device.  Independent of the other headers of this project: this one includes none of them and the
 * library links none of their libraries.
 */
#ifndef SIMRANK_DENSITY_H
#define SIMRANK_DENSITY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_DENSITY_VERSION 1
#define SIMRANK_DENSITY_MAX_LEVELS 8        /* thresholds of one degrees sweep: their pass masks share 8 KiB of LDS */
#define SIMRANK_DENSITY_TILE 64             /* a tile is 64 x 64 entries: one 64-bit pass mask per row and level */
#define SIMRANK_DENSITY_NONE 0x7fffffff     /* attach[x] of a node no core node has claimed */

#if defined(__GNUC__)
#define SIMRANK_DENSITY_API __attribute__((visibility("default")))
#else
#define SIMRANK_DENSITY_API
#endif

enum {
    SIMRANK_DENSITY_OK = 0,
    SIMRANK_DENSITY_ERR_INVALID = -1,      /* bad argument: NULL, shape, layout, levels */
    SIMRANK_DENSITY_ERR_HIP = -2           /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_DENSITY_PANEL_F32 = 0,         /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_DENSITY_ROWMAJOR_F32 = 1,      /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_DENSITY_PANEL_F16 = 2,         /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_DENSITY_ROWMAJOR_F64 = 3       /* float64 row-major: (r, c) at r * stride + c */
};

/* bits of *status (0 = every walk ended at a root) */
enum {
    SIMRANK_DENSITY_BAD_PARENT = 1,        /* a parent above its node, or a parent or an attachment outside 0 .. n - 1 */
    SIMRANK_DENSITY_CAP_REACHED = 2        /* a walk or a retry loop reached its cap of n + 8 steps */
};

SIMRANK_DENSITY_API int simrank_density_version(void);
SIMRANK_DENSITY_API const char* simrank_density_last_error(void);

/* deg[l * n + i] = 0 for l < n_levels (1 .. SIMRANK_DENSITY_MAX_LEVELS), i < n (0 <= n < 2^31 - 8); parent[i] = i;
 * attach[i] = SIMRANK_DENSITY_NONE; *status = 0.  `deg`: device int32 [n_levels][n]; `parent`, `attach`: device int32
 * [n], or both NULL when only degrees are wanted; `status`: one device int32.  Asynchronous on `stream`. */
SIMRANK_DENSITY_API int simrank_density_init(int32_t* deg, int32_t* parent, int32_t* attach, int64_t n, int32_t n_levels,
                                             int32_t* status, void* stream);

/* The SQUARE block S of n x n values, position p being the node ids[p] (NULL: p itself): for every position a whose id
 * is a node and every level l, deg[l * n + id(a)] += the number of positions b != a whose id is a node with
 * v(a, b) >= edges[l] or v(b, a) >= edges[l].  `edges`: device array of n_levels thresholds in the type they are
 * compared in: float for the f32 layouts and for binary16 (read as (float)h * 2^-14), double for float64.  One workgroup
 * per pair of 64 x 64 tiles (I, J), I <= J: each row of tile (I, J) and of tile (J, I) becomes one 64-bit pass mask per
 * level (a wave's ballot) in LDS, the second tile's bit matrix is read transposed, ORed with the first and counted per
 * row, and the other way round per column; every element is read once, 64-bit offsets throughout, and integer atomic
 * adds are the only atomics.  Asynchronous on `stream`. */
SIMRANK_DENSITY_API int simrank_density_degrees(const void* S, int32_t layout, int64_t stride, int64_t n, const int32_t* ids,
                                                const void* edges, int32_t n_levels, int32_t* deg, void* stream);

/* Every entry v >= *edge of the block with id(r) != id(c), both ids in 0 .. n - 1: both nodes core
 * (deg[x] >= min_neighbors >= 0) -> united; one of them core -> an atomic minimum of the core node into the other's
 * `attach`; neither -> nothing.  `edge`: ONE device threshold, in the type simrank_density_degrees compares in; `deg`:
 * device int32 [n], one level of the counters, only read; `parent`, `attach` and `status` as simrank_density_init left
 * them or as earlier calls of this entry did.  A sweep of 16-byte loads along the contiguous direction of the layout, as
 * simrank_cluster_union's.  Asynchronous on `stream`. */
SIMRANK_DENSITY_API int simrank_density_union(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                              const int32_t* row_ids, const int32_t* col_ids, const void* edge,
                                              const int32_t* deg, int32_t min_neighbors, int32_t* parent, int32_t* attach,
                                              int64_t n, int32_t* status, void* stream);

/* labels[i] = the root of i when deg[i] >= min_neighbors (the smallest core node of its cluster, once every block went
 * through simrank_density_union); else the root of attach[i] when a core node claimed i (a border node: the cluster of
 * its smallest core neighbour); else -1 (noise).  `labels`: device int32 [n], none of the other arrays.  `parent`,
 * `attach` and `deg` are only read.  Asynchronous on `stream`. */
SIMRANK_DENSITY_API int simrank_density_labels(const int32_t* parent, const int32_t* attach, const int32_t* deg,
                                               int32_t min_neighbors, int64_t n, int32_t* labels, int32_t* status,
                                               void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_DENSITY_H */
