/*
 * simrank_groups.h — a clustering of a similarity iterate scored where the iterate lies (libsimrank_groups.so).
 *
 * Given a labelling of the nodes into groups, how similar is every node to every group: one sweep of a block of the
 * iterate IN PLACE, a (row, group) mean at a time, and per row three numbers:
 *
 *     own        the mean similarity of the row's node to the OTHER members of its own group
 *     other      the best mean similarity of the row's node to another group
 *     nearest    that group
 *
 * and, when asked for, every mean.  The definitions, all part of the contract.  For the row r of a node and a group g,
 * M = the entries of g's list but the block column row_col[r] (the row's own node, left out of every sum):
 *
 *     sum(r, g)   the sum of S[r][c] over M, each element widened as simrank_query.h's rows widen it (a float, binary16 as
 *                 (float)h * 2^-14, a double) and then to double; accumulated in double from +0.0, so a sum of zeros of
 *                 either sign is +0.0
 *     mean(r, g)  sum / |M| (one correctly rounded division); NaN when M is empty
 *     own         mean(r, row_group[r])
 *     other       the first of the mean(r, g), g != row_group[r], in the order (mean descending, g ascending); a NaN mean
 *                 is never chosen; nearest = g.  No candidate: nearest = -1 and other = NaN
 *
 * A NaN entry makes its (row, group) mean NaN.  A position of a list outside 0 .. n_cols - 1 reads NaN: no load leaves
 * the block, and padding columns are read only if a list names them.
 *
 * Rounding.  The order of the double additions of a (row, group) sum is a function of the group's length alone: a list
 * of at most 8 positions is added in list order by one lane; a longer one by a wave (below 1024) or the workgroup (from
 * 1024 on) with a fixed lane stride, four running sums a lane, and a fixed tree over the lanes and the waves.  There are no
 * floating-point atomics: two runs give the same bits, and |sum - exact| <= |M| * 2^-52 * (the sum of |S[r][c]| over M).
 *
 * A block of n_rows x n_cols values is read as the plans of simrank_hip.h report it, in one of the four layouts below.
 *
 * Conventions as simrank_cluster.h: 0 or a negative status code (SIMRANK_GROUPS_ERR_*), the message of the last failure
 * on the calling thread from simrank_groups_last_error(); device pointers are HIP device memory of the current device;
 * `stream` is a hipStream_t passed as void*; the entry only queues work on it and allocates nothing.  Argument checks
 * need no device.  Independent of the other headers of this project: this one includes none of them and the library
 * links none of their libraries.
 */
#ifndef SIMRANK_GROUPS_H
#define SIMRANK_GROUPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_GROUPS_VERSION 1
#define SIMRANK_GROUPS_LANE_MAX 8           /* a list of at most this many positions is summed by one lane, in list order */
#define SIMRANK_GROUPS_WAVE_MAX 1023        /* a longer one of at most this many by one wave; beyond, by the workgroup */

#if defined(__GNUC__)
#define SIMRANK_GROUPS_API __attribute__((visibility("default")))
#else
#define SIMRANK_GROUPS_API
#endif

enum {
    SIMRANK_GROUPS_OK = 0,
    SIMRANK_GROUPS_ERR_INVALID = -1,       /* bad argument: NULL, shape, layout, stride, groups */
    SIMRANK_GROUPS_ERR_HIP = -2            /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_GROUPS_PANEL_F32 = 0,          /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_GROUPS_ROWMAJOR_F32 = 1,       /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_GROUPS_PANEL_F16 = 2,          /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_GROUPS_ROWMAJOR_F64 = 3        /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_GROUPS_API int simrank_groups_version(void);
SIMRANK_GROUPS_API const char* simrank_groups_last_error(void);

/* The means of every row of the block to every group, as defined above.  All arrays are device memory.
 *     row_group  int32 [n_rows]: the group (0 .. n_groups - 1) of the node in row r; < 0: the row is skipped and its
 *                outputs are left untouched
 *     row_col    int32 [n_rows]: the block column that holds row r's own node, left out of every sum; -1: none
 *     col_pos    int32 [group_ptr[n_groups]]: block column positions, group-major, in any order within a group
 *     group_ptr  int64 [n_groups + 1]: ascending offsets into col_pos, group_ptr[0] = 0; n_groups >= 1
 *     own, other double [n_rows]; nearest int32 [n_rows]
 *     means      NULL, or double [n_rows][ld_means] (ld_means >= n_groups): means[r * ld_means + g] = mean(r, g); the
 *                elements from n_groups on are left untouched
 * Shapes are below 2^31; element offsets are 64-bit throughout.  A block must start on a multiple of its element's size.
 * One workgroup per row walks the groups in order; nothing but the outputs is written.  Asynchronous on `stream`. */
SIMRANK_GROUPS_API int simrank_groups_means(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                            const int32_t* row_group, const int32_t* row_col, const int32_t* col_pos,
                                            const int64_t* group_ptr, int32_t n_groups, double* own, double* other,
                                            int32_t* nearest, double* means, int64_t ld_means, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_GROUPS_H */
