/*
 * simrank_kmedoids.h — the two device steps of a k-medoids alternation on a similarity iterate (libsimrank_kmedoids.so).
 *
 * K medoids, each a row of a block of the iterate read IN PLACE, and the n_cols nodes that are the block's columns:
 *
 *     assign     every column goes to the medoid whose row holds the largest value in it
 *     pick       every cluster's medoid moves to the member with the largest `own` (the mean similarity to the other
 *                members of its cluster, as simrank_groups.h computes it), if that is strictly larger than the medoid's
 *
 * The definitions, all part of the contract.
 *
 *     v(j, c)    the element S[med_row[j]][c], widened as simrank_query.h's rows widen it (a float, binary16 as
 *                (float)h * 2^-14, a double) and then to double; NaN when med_row[j] is outside 0 .. n_rows - 1: no load
 *                leaves the block
 *     order      candidates are compared in double in the order (v descending, j ascending): the first j wins a tie,
 *                -0.0 equals +0.0, and a NaN is never a candidate
 *
 * assign.  best(c) is the first candidate j of column c in that order.  Without `current`, or where current[c] is outside
 * 0 .. K - 1: cluster[c] = best(c), or 0 when the column has no candidate.  With current[c] = k: the column moves to
 * best(c) iff v(best(c), c) > v(k, c), or v(k, c) is NaN and a candidate exists; otherwise it stays in k.  A column that
 * is a medoid's own node (med_col[j] = c) is cluster j whatever its values say (the first such j when several name it).
 * value[c] = v(cluster[c], c) with the bits as widened (some NaN where that is one).  *moved grows by the number of columns with
 * cluster[c] != current[c]; by n_cols without `current`.
 *
 * pick.  The members of cluster j are the positions col_pos[group_ptr[j] .. group_ptr[j + 1]), the lists
 * simrank_groups_means takes; a position outside 0 .. n_rows - 1 is skipped.  The candidate is the member with the largest
 * own[position], the earliest in the list on a tie; a NaN is no candidate.  With m = med_row[j] and own(m) NaN when m is
 * outside 0 .. n_rows - 1: med_row[j] becomes the candidate's position iff own(candidate) > own(m), or own(m) is NaN and
 * there is a candidate.  cohesion[j] = own of the medoid the call leaves; NaN for an empty list, whose medoid stays.
 * *changed grows by the number of clusters whose med_row changed.
 *
 * No floating-point value is added anywhere: both entries compare and copy, there are no floating-point atomics (the two
 * counters are integer atomics) and two runs give the same bits.
 *
 * A block of n_rows x n_cols values is read as the plans of simrank_hip.h report it, in one of the four layouts below.
 *
 * Conventions as simrank_groups.h: 0 or a negative status code (SIMRANK_KMEDOIDS_ERR_*), the message of the last failure
 * on the calling thread from simrank_kmedoids_last_error(); device pointers are HIP device memory of the current device;
 * `stream` is a hipStream_t passed as void*; an entry only queues work on it and allocates nothing.  Argument checks
 * need no device.  Independent of the other headers of this project: this one includes none of them and the library
 * links none of their libraries.
 */
#ifndef SIMRANK_KMEDOIDS_H
#define SIMRANK_KMEDOIDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_KMEDOIDS_VERSION 1
#define SIMRANK_KMEDOIDS_CHUNK 1024          /* block columns of one workgroup of simrank_kmedoids_assign */

#if defined(__GNUC__)
#define SIMRANK_KMEDOIDS_API __attribute__((visibility("default")))
#else
#define SIMRANK_KMEDOIDS_API
#endif

enum {
    SIMRANK_KMEDOIDS_OK = 0,
    SIMRANK_KMEDOIDS_ERR_INVALID = -1,     /* bad argument: NULL, shape, layout, stride, K */
    SIMRANK_KMEDOIDS_ERR_HIP = -2          /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_KMEDOIDS_PANEL_F32 = 0,        /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_KMEDOIDS_ROWMAJOR_F32 = 1,     /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_KMEDOIDS_PANEL_F16 = 2,        /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_KMEDOIDS_ROWMAJOR_F64 = 3      /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_KMEDOIDS_API int simrank_kmedoids_version(void);
SIMRANK_KMEDOIDS_API const char* simrank_kmedoids_last_error(void);

/* The assignment step, as defined above.  All arrays are device memory.
 *     med_row   int32 [K]: the block row of medoid j; a row outside 0 .. n_rows - 1 reads NaN
 *     med_col   int32 [K]: the block column that is medoid j's own node; -1 (or any column outside the block): none
 *     current   NULL (the first assignment), or int32 [n_cols]: the cluster every column is in
 *     cluster   int32 [n_cols], value double [n_cols]: outputs; `cluster` may not overlap `current`
 *     moved     NULL, or one uint32 the call ADDS to (an integer atomic)
 * K >= 1.  Shapes are below 2^31; element offsets are 64-bit throughout.  A block must start on a multiple of its
 * element's size.  One workgroup per SIMRANK_KMEDOIDS_CHUNK columns reads the K rows' elements of its columns, K x n_cols
 * elements in all; nothing but the outputs is written.  Asynchronous on `stream`. */
SIMRANK_KMEDOIDS_API int simrank_kmedoids_assign(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                                 const int32_t* med_row, const int32_t* med_col, int32_t K,
                                                 const int32_t* current, int32_t* cluster, double* value, uint32_t* moved,
                                                 void* stream);

/* The update step, as defined above.  All arrays are device memory.
 *     own        double [n_rows]: indexed by block row (in a block whose row r and column r are one node, by position)
 *     col_pos    int32 [group_ptr[K]]: positions, cluster-major; a tie goes to the earliest in a list
 *     group_ptr  int64 [K + 1]: ascending offsets into col_pos, group_ptr[0] = 0
 *     med_row    int32 [K]: in and out
 *     cohesion   double [K]: output
 *     changed    NULL, or one uint32 the call ADDS to (an integer atomic)
 * K >= 1, n_rows below 2^31.  One wave per cluster.  Asynchronous on `stream`. */
SIMRANK_KMEDOIDS_API int simrank_kmedoids_pick(const double* own, int64_t n_rows, const int32_t* col_pos,
                                               const int64_t* group_ptr, int32_t K, int32_t* med_row, double* cohesion,
                                               uint32_t* changed, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_KMEDOIDS_H */
