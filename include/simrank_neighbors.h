/*
 * simrank_neighbors.h — a kept model as per-node neighbour lists (libsimrank_neighbors.so).
 *
 * The pruned form of one side of a model of n nodes with k kept neighbours per node is three device arrays:
 *
 *     nbr_ids   int32  [n][k]   ids (caller positions 0 .. n - 1) of node a's k most similar OTHER nodes, in the total
 *                               order (value descending, id ascending); slots past the candidates hold -1
 *     nbr_vals  double [n][k]   their values, widened as simrank_query_rows widens them; 0 in the empty slots
 *     diag      double [n]      S[a][a]
 *
 * They stand for the matrix P that holds the kept entries, the diagonal, and +0.0 everywhere else (P is in general NOT
 * symmetric: row a is node a's list).
 *
 *     simrank_neighbors_select   builds the lists: the k best of chosen rows of a block of an iterate read IN PLACE in one
 *                                of the four layouts below; same arguments and same result as simrank_query_topk, at a
 *                                cost that does not grow with k
 *     simrank_neighbors_rows     dense float64 rows of P
 *     simrank_neighbors_pairs    P[a_i][b_i] per pair
 *     simrank_neighbors_score    the band simrank_sets_score would write for P: sum_e w_e * P[pos_e][b], float64, in list
 *                                order, every product and every sum rounded separately (no fused multiply-add)
 *
 * Conventions as simrank_query.h: 0 or a negative status (SIMRANK_NEIGHBORS_ERR_*), the message of the last failure on
 * the calling thread from simrank_neighbors_last_error(); device pointers are HIP device memory of the current device;
 * `stream` is a hipStream_t passed as void*; every entry point only queues work on it and allocates nothing (the
 * selection keeps its scratch in the workgroup's local memory: there is no workspace to pass).  Argument checks need no
 * device.  Independent of the other headers of this project: this one includes none of them and the library links none
 * of their libraries.
 */
#ifndef SIMRANK_NEIGHBORS_H
#define SIMRANK_NEIGHBORS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_NEIGHBORS_VERSION 1
#define SIMRANK_NEIGHBORS_MAX_K 4096       /* the longest list: k survivors of a row are sorted in local memory */
#define SIMRANK_NEIGHBORS_CHUNK 2048       /* output columns of one workgroup of _rows and _score: 256 lanes x 8 */
#define SIMRANK_NEIGHBORS_MAX_BLOCKS (1 << 24)   /* workgroups of one call of _rows and _score */

#if defined(__GNUC__)
#define SIMRANK_NEIGHBORS_API __attribute__((visibility("default")))
#else
#define SIMRANK_NEIGHBORS_API
#endif

enum {
    SIMRANK_NEIGHBORS_OK = 0,
    SIMRANK_NEIGHBORS_ERR_INVALID = -1,    /* bad argument: NULL, shape, layout, k, too many workgroups */
    SIMRANK_NEIGHBORS_ERR_HIP = -2         /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_NEIGHBORS_PANEL_F32 = 0,       /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_NEIGHBORS_ROWMAJOR_F32 = 1,    /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_NEIGHBORS_PANEL_F16 = 2,       /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_NEIGHBORS_ROWMAJOR_F64 = 3     /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_NEIGHBORS_API int simrank_neighbors_version(void);
SIMRANK_NEIGHBORS_API const char* simrank_neighbors_last_error(void);

/* The k best of n_q chosen rows of a block, what simrank_query_topk returns for the same arguments:
 *     idx_out[q * k + j], val_out[q * k + j]   j-th best of row row_pos[q] in the order (value descending, id ascending)
 * id(c) = col_ids[c] (device int32, distinct ids >= 0), or c when col_ids is NULL; the column whose id is row_ids[q] (the
 * row's own node) is no candidate, NaN is none either; -0.0 and +0.0 tie and each keeps its own bits; slots past the
 * candidates hold id -1 and value 0; a row position outside the block has no candidates.  1 <= k <=
 * SIMRANK_NEIGHBORS_MAX_K.  One workgroup per row: a radix select (11-bit digits, histograms in local memory) on an
 * order-preserving integer key of the value, then on the id among the ties of the k-th value, one collecting sweep and a
 * sort of the k survivors in local memory.  A row is swept at most 4 + 3 times from f32 and binary16 (7 + 3 from
 * float64) whatever k is, fewer when a digit already separates the k-th. */
SIMRANK_NEIGHBORS_API int simrank_neighbors_select(const void* S, int32_t layout, int64_t stride, int64_t n_rows,
                                                   int64_t n_cols, const int32_t* row_pos, const int32_t* row_ids,
                                                   int64_t n_q, const int32_t* col_ids, int32_t k, int32_t* idx_out,
                                                   double* val_out, void* stream);

/* out[q * ld_out + b] = P[row_pos[q]][b] for q < n_q and b < n: zero (+0.0), the list's entries at their ids, the
 * diagonal.  A row position outside 0 .. n - 1 gives a row of NaN; a list id outside 0 .. n - 1 is an empty slot.  One
 * workgroup owns one query row and SIMRANK_NEIGHBORS_CHUNK columns, builds them in local memory and writes them with
 * coalesced 8-byte stores. */
SIMRANK_NEIGHBORS_API int simrank_neighbors_rows(const int32_t* nbr_ids, const double* nbr_vals, const double* diag,
                                                 int64_t n, int32_t k, const int32_t* row_pos, int64_t n_q, double* out,
                                                 int64_t ld_out, void* stream);

/* out[i] = P[a_pos[i]][b_pos[i]]: the diagonal from diag, a listed neighbour's value, +0.0 for an absent entry, NaN for
 * a position outside 0 .. n - 1. */
SIMRANK_NEIGHBORS_API int simrank_neighbors_pairs(const int32_t* nbr_ids, const double* nbr_vals, const double* diag,
                                                  int64_t n, int32_t k, const int32_t* a_pos, const int32_t* b_pos,
                                                  int64_t n_pairs, double* out, void* stream);

/* The band simrank_sets_score writes, for P: for every basket q < n_sets and column b < n
 *     out[q * ld_out + b] = sum_{e = set_ptr[q] .. set_ptr[q + 1] - 1} set_w[e] * P[set_pos[e]][b]
 * float64, members strictly in list order, every product and every sum rounded separately.  An absent entry of P adds an
 * exact zero to a sum that starts at +0.0 and so never is -0.0: it is skipped, with the same bits for finite weights.
 * set_ptr: device int64 [n_sets + 1]; set_pos: device int32 node positions; set_w: device double.  excl_ptr (device int64
 * [n_sets + 1]) and excl_cols (device int32 columns), or both NULL: the listed columns of basket q receive -inf.  An
 * empty basket scores 0.  A list position outside 0 .. n - 1 is not read: it poisons every sum of its basket with NaN.
 * One workgroup owns one basket and SIMRANK_NEIGHBORS_CHUNK columns, whose sums it keeps in local memory. */
SIMRANK_NEIGHBORS_API int simrank_neighbors_score(const int32_t* nbr_ids, const double* nbr_vals, const double* diag,
                                                  int64_t n, int32_t k, const int64_t* set_ptr, const int32_t* set_pos,
                                                  const double* set_w, int64_t n_sets, const int64_t* excl_ptr,
                                                  const int32_t* excl_cols, double* out, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_NEIGHBORS_H */
