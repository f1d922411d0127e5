/*
 * simrank_explain.h — which neighbour pairs make two nodes similar: the device half (libsimrank_explain.so).
 *
 * The update of SimRank gives a pair (a, b) a sum over the pairs of their neighbours, sum_{i in I(a)} sum_{j in I(b)}
 * S[i, j].  For a band of pairs this library
 *
 *     gather     copies, per pair, the sub-matrix S[I(a), I(b)] of a block of the iterate read IN PLACE into a float64
 *                piece of a device band
 *     reduce     adds up, per pair, the piece's rows, its columns and all of it, and counts its contributors
 *     select     finds, per pair, the k largest contributors of the piece
 *
 * The definitions, all part of the contract.
 *
 *     lists      pair p has the row list a_pos[a_ptr[p] .. a_ptr[p + 1]) of na entries and the column list
 *                b_pos[b_ptr[p] .. b_ptr[p + 1]) of nb entries: positions in the block, repeats allowed
 *     piece      na x nb doubles, row-major, at band + band_ptr[p]; band_ptr[p + 1] - band_ptr[p] = na * nb (a pair for
 *                which that does not hold is skipped by every entry: nothing of it is read or written)
 *     x(i, j)    the element S[a_pos[a_ptr[p] + i]][b_pos[b_ptr[p] + j]], widened as simrank_query.h's rows widen it (a
 *                float, binary16 as (float)h * 2^-14, a double) and then to double; NaN when either position is outside
 *                the block: no load leaves the block
 *     contributor  an element of a piece that is neither NaN nor a zero of either sign
 *     order      contributors are compared in the order (value descending, i ascending, j ascending), i and j being
 *                the indices WITHIN the two lists
 *
 * reduce.  row_sum[a_ptr[p] + i] = sum_j x(i, j), col_sum[b_ptr[p] + j] = sum_i x(i, j), raw[p] = sum_i row_sum[..+ i]
 * (the sum of the row sums, not a second sum of the elements), contributors[p] = the count.  Every sum is float64; the
 * order of its additions depends on na and nb alone, and there are no floating-point atomics (the count is an integer
 * atomic): two runs give the same bits.  A sum of m terms lies within m * 2^-52 * sum |x| of the exact one.  NaN
 * propagates.  An empty sum is +0.0.
 *
 * select.  best_i / best_j / best_value [p * k + r] for r < k: the r-th contributor of pair p in the order above; slots
 * past the contributors hold -1 / -1 / 0.0.  Values are copied with their bits.  The entry compares and copies, nothing
 * is added.
 *
 * A block of n_rows x n_cols values is read as the plans of simrank_hip.h report it, in one of the four layouts below.
 *
 * Conventions as simrank_kmedoids.h: 0 or a negative status code (SIMRANK_EXPLAIN_ERR_*), the message of the last
 * failure on the calling thread from simrank_explain_last_error(); device pointers are HIP device memory of the current
 * device; `stream` is a hipStream_t passed as void*; an entry only queues work on it and allocates nothing.  Argument
 * checks need no device.  Independent of the other headers of this project: this one includes none of them and the
 * library links none of their libraries.
 */
#ifndef SIMRANK_EXPLAIN_H
#define SIMRANK_EXPLAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_EXPLAIN_VERSION 1
#define SIMRANK_EXPLAIN_MAX_K 1024           /* the largest k of simrank_explain_select */

#if defined(__GNUC__)
#define SIMRANK_EXPLAIN_API __attribute__((visibility("default")))
#else
#define SIMRANK_EXPLAIN_API
#endif

enum {
    SIMRANK_EXPLAIN_OK = 0,
    SIMRANK_EXPLAIN_ERR_INVALID = -1,      /* bad argument: NULL, shape, layout, stride, k */
    SIMRANK_EXPLAIN_ERR_HIP = -2           /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_EXPLAIN_PANEL_F32 = 0,         /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_EXPLAIN_ROWMAJOR_F32 = 1,      /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_EXPLAIN_PANEL_F16 = 2,         /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_EXPLAIN_ROWMAJOR_F64 = 3       /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_EXPLAIN_API int simrank_explain_version(void);
SIMRANK_EXPLAIN_API const char* simrank_explain_last_error(void);

/* The pieces of n_pairs pairs, as defined above.  All arrays are device memory.
 *     a_pos, b_pos   int32: the lists, pair after pair
 *     a_ptr, b_ptr   int64 [n_pairs + 1]: ascending offsets into them (the first need not be 0: a band of a longer call
 *                    passes the call's arrays and its own part of the offsets)
 *     band_ptr       int64 [n_pairs + 1]: ascending offsets into band, in elements
 *     max_terms      the largest na * nb of the call (or more): it sizes the launch and nothing else; a larger piece is
 *                    still written whole
 *     band           double [band_ptr[n_pairs]]: output
 * n_pairs is below 2^31 and may be 0.  Shapes are below 2^31; element offsets are 64-bit throughout.  A block must start
 * on a multiple of its element's size.  One element is read per element written; nothing but the band is written.
 * Asynchronous on `stream`. */
SIMRANK_EXPLAIN_API int simrank_explain_gather(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                               const int32_t* a_pos, const int64_t* a_ptr, const int32_t* b_pos,
                                               const int64_t* b_ptr, const int64_t* band_ptr, int64_t n_pairs,
                                               int64_t max_terms, double* band, void* stream);

/* The sums and the count of every piece, as defined above.  All arrays are device memory.
 *     max_rows, max_cols   the largest na and nb of the call (or more): they size the launch and nothing else
 *     row_sum        double [a_ptr[n_pairs]], col_sum double [b_ptr[n_pairs]], raw double [n_pairs],
 *     contributors   int64 [n_pairs]: outputs
 * Asynchronous on `stream`. */
SIMRANK_EXPLAIN_API int simrank_explain_reduce(const double* band, const int64_t* a_ptr, const int64_t* b_ptr,
                                               const int64_t* band_ptr, int64_t n_pairs, int64_t max_rows, int64_t max_cols,
                                               double* row_sum, double* col_sum, double* raw, int64_t* contributors,
                                               void* stream);

/* The k best contributors of every piece, as defined above.  All arrays are device memory.
 *     best_i, best_j   int32 [n_pairs * k], best_value double [n_pairs * k]: outputs
 * 1 <= k <= SIMRANK_EXPLAIN_MAX_K.  One workgroup per pair.  Asynchronous on `stream`. */
SIMRANK_EXPLAIN_API int simrank_explain_select(const double* band, const int64_t* a_ptr, const int64_t* b_ptr,
                                               const int64_t* band_ptr, int64_t n_pairs, int32_t k, int32_t* best_i,
                                               int32_t* best_j, double* best_value, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_EXPLAIN_H */
