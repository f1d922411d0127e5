/*
 * simrank_sets.h — basket queries on an iterate that stays on the device (libsimrank_sets.so).
 *
 * A basket q is a list of fitted nodes with one weight each.  Its score row is
 *
 *     score(q, b) = sum_{e in list q} w_e * S[pos(e)][b]
 *
 * accumulated in float64 IN LIST ORDER, every product and every sum rounded separately (no fused multiply-add), each
 * element widened as simrank_query_rows widens it (f32 -> double; binary16 h -> (float)h * 2^-14 -> double; float64 as it
 * is).  A host loop `acc = 0.0; for e: acc = acc + (w_e * s_e)` in IEEE double reproduces every value bit for bit.
 *
 *     simrank_sets_score   the score rows of n_sets baskets over one column block of the iterate, read IN PLACE in one of
 *                          the four layouts below, as a float64 row-major band; listed columns of a basket are marked
 *                          -inf ("no candidate")
 *     simrank_sets_topk    the k best of each row of such a band in the total order (score descending, id ascending);
 *                          -inf and NaN are never picked
 *
 * Conventions as simrank_query.h: 0 or a negative status (SIMRANK_SETS_ERR_*), the message of the last failure on the
 * calling thread from simrank_sets_last_error(); device pointers are HIP device memory of the current device; `stream` is
 * a hipStream_t passed as void*; every entry point only queues work on it and allocates nothing.  A list position outside
 * the block's rows or a mapped column outside its columns is not read: it poisons the sums it belongs to with NaN.
 * Independent of the other headers of this project: this one includes none of them and the library links none of their
 * libraries.
 */
#ifndef SIMRANK_SETS_H
#define SIMRANK_SETS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_SETS_VERSION 1
#define SIMRANK_SETS_CHUNK 1024        /* output columns of one workgroup: 256 lanes x 4 */
#define SIMRANK_SETS_MAX_BLOCKS (1 << 24)   /* workgroups of one call: 2^32 work-items are never reached */

#if defined(__GNUC__)
#define SIMRANK_SETS_API __attribute__((visibility("default")))
#else
#define SIMRANK_SETS_API
#endif

enum {
    SIMRANK_SETS_OK = 0,
    SIMRANK_SETS_ERR_INVALID = -1,     /* bad argument: NULL, shape, layout, too many workgroups */
    SIMRANK_SETS_ERR_HIP = -2          /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_SETS_PANEL_F32 = 0,        /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_SETS_ROWMAJOR_F32 = 1,     /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_SETS_PANEL_F16 = 2,        /* IEEE binary16 holding value x 2^14, 64-column panels:
                                          (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_SETS_ROWMAJOR_F64 = 3      /* float64 row-major: (r, c) at r * stride + c */
};

/* how the workgroups of simrank_sets_score are numbered (the same values either way) */
enum {
    SIMRANK_SETS_GRID_BASKET_MAJOR = 0,    /* the chunks of a basket follow each other */
    SIMRANK_SETS_GRID_CHUNK_LABEL = 1      /* every workgroup of a column chunk, over all baskets, carries the same
                                              blockIdx % 8 (fewer than 8 chunks: the labels are divided among them) */
};

SIMRANK_SETS_API int simrank_sets_version(void);
SIMRANK_SETS_API const char* simrank_sets_last_error(void);

/* Workgroups simrank_sets_score launches for n_sets baskets over n_out output columns in `grid_order`; -1 for bad
 * arguments.  A caller cuts its baskets into bands so that this stays at or below SIMRANK_SETS_MAX_BLOCKS. */
SIMRANK_SETS_API int64_t simrank_sets_blocks(int64_t n_sets, int64_t n_out, int32_t grid_order);

/* For every basket q < n_sets and output column j < n_out:
 *     out[q * ld_out + j] = sum_{e = set_ptr[q] .. set_ptr[q + 1] - 1} set_w[e] * S[set_pos[e]][col(j)]
 * in the order and rounding stated above; col(j) = col_pos[j], or j when col_pos is NULL (then n_out <= n_cols).
 * set_ptr: device int64 [n_sets + 1], ascending; set_pos: device int32, ROW POSITIONS of the block (the solver's order);
 * set_w: device double.  excl_ptr (device int64 [n_sets + 1]) and excl_cols (device int32 OUTPUT columns j), or both
 * NULL: the listed columns of basket q receive -inf instead (entries outside 0 .. n_out - 1 mark nothing).  An empty
 * basket scores 0.  One workgroup owns one basket and SIMRANK_SETS_CHUNK output columns; without col_pos a lane loads 16
 * bytes (8 of binary16, 2 x 16 of float64) of each member's row, several members in flight. */
SIMRANK_SETS_API int simrank_sets_score(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                        const int32_t* col_pos, int64_t n_out, const int64_t* set_ptr,
                                        const int32_t* set_pos, const double* set_w, int64_t n_sets,
                                        const int64_t* excl_ptr, const int32_t* excl_cols, double* out, int64_t ld_out,
                                        int32_t grid_order, void* stream);

/* The k best of every row of a float64 row-major band (device double, n_sets rows of n_out values, ld_band apart):
 *     idx_out[q * k + j], val_out[q * k + j]   j-th best of row q in the order (value descending, id ascending)
 * id(c) = col_ids[c] (device int32, ids >= 0), or c when col_ids is NULL.  -inf and NaN are no candidates; slots past the
 * candidates hold id -1 and value 0.  One wave per row, k passes over it: the cost is k * n_out reads per row. */
SIMRANK_SETS_API int simrank_sets_topk(const double* band, int64_t ld_band, int64_t n_sets, int64_t n_out,
                                       const int32_t* col_ids, int32_t k, int32_t* idx_out, double* val_out,
                                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_SETS_H */
