/*
 * simrank_candidates.h — the k best of chosen rows of a kept model among a LIST of candidate columns
 * (libsimrank_candidates.so).
 *
 * simrank_query_topk and simrank_neighbors_select rank a row against every column of a block.  A deployed model is asked
 * for the best among the items in stock, in a category, not yet shown: a subset of the columns, the same for every query
 * of a call.  simrank_candidates_topk selects among the listed columns only, reading the block IN PLACE in one of the
 * four layouts below, and fetches each candidate's element once per query.
 *
 * Conventions as simrank_neighbors.h: 0 or a negative status (SIMRANK_CANDIDATES_ERR_*), the message of the last failure
 * on the calling thread from simrank_candidates_last_error(); device pointers are HIP device memory of the current
 * device; `stream` is a hipStream_t passed as void*; every entry point only queues work on it and allocates nothing (the
 * selection keeps its scratch in the workgroup's local memory: there is no workspace to pass).  Argument checks need no
 * device.  Independent of the other headers of this project: this one includes none of them and the library links none
 * of their libraries.
 */
#ifndef SIMRANK_CANDIDATES_H
#define SIMRANK_CANDIDATES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_CANDIDATES_VERSION 1
#define SIMRANK_CANDIDATES_MAX_K 4096             /* the most picks: k survivors of a row are sorted in local memory */
#define SIMRANK_CANDIDATES_MAX_BLOCKS (1 << 16)   /* workgroups of one call; a workgroup strides over the queries */

#if defined(__GNUC__)
#define SIMRANK_CANDIDATES_API __attribute__((visibility("default")))
#else
#define SIMRANK_CANDIDATES_API
#endif

enum {
    SIMRANK_CANDIDATES_OK = 0,
    SIMRANK_CANDIDATES_ERR_INVALID = -1,   /* bad argument: NULL, shape, layout, k */
    SIMRANK_CANDIDATES_ERR_HIP = -2        /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_CANDIDATES_PANEL_F32 = 0,      /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_CANDIDATES_ROWMAJOR_F32 = 1,   /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_CANDIDATES_PANEL_F16 = 2,      /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_CANDIDATES_ROWMAJOR_F64 = 3    /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_CANDIDATES_API int simrank_candidates_version(void);
SIMRANK_CANDIDATES_API const char* simrank_candidates_last_error(void);

/* The k best of n_q chosen rows of a block among n_cand listed columns:
 *     idx_out[q * k + j], val_out[q * k + j]   j-th best candidate of row row_pos[q]
 * The candidate at list index i is block column cand_pos[i] (device int32); its id is cand_ids[i] (device int32), or
 * cand_pos[i] when cand_ids is NULL.  The order is value descending, ties by LIST INDEX ascending: a caller that passes
 * the list in ascending id order gets the project's total order (value descending, id ascending), and with every column
 * listed that way what simrank_neighbors_select returns for the same block.  The values follow that entry point's
 * rules: the candidate whose id is row_ids[q] (the row's own node) is no candidate, NaN is none either; -0.0 and +0.0
 * tie and each keeps its own bits in val_out; values are widened as simrank_query_rows widens them; slots past the
 * candidates hold id -1 and value 0; a row position outside the block has no candidates.  A cand_pos[i] outside
 * 0 .. n_cols - 1 is not read and is no candidate.  n_cand = 0 is allowed (every slot is empty; cand_pos may be NULL);
 * 1 <= k <= SIMRANK_CANDIDATES_MAX_K; n_q = 0 returns OK and launches nothing; n_q, n_cand, n_rows and n_cols are below
 * 2^31.
 *
 * One workgroup of 256 per query row, min(n_q, SIMRANK_CANDIDATES_MAX_BLOCKS) workgroups striding over the rows.  While
 * n_cand <= simrank_candidates_staged(layout) a workgroup gathers its row's candidates ONCE, keeps their
 * order-preserving integer keys in local memory and runs the radix select (11-bit digits) on the key and then on the
 * list index among the ties of the k-th value there; above that it gathers again in every pass, as
 * simrank_neighbors_select does.  The k survivors are sorted in local memory and their elements read once more for
 * val_out (a key folds the two zeros).  The local memory of a call grows with n_cand and k, not with the caps. */
SIMRANK_CANDIDATES_API int simrank_candidates_topk(const void* S, int32_t layout, int64_t stride, int64_t n_rows,
                                                   int64_t n_cols, const int32_t* row_pos, const int32_t* row_ids,
                                                   int64_t n_q, const int32_t* cand_pos, const int32_t* cand_ids,
                                                   int64_t n_cand, int32_t k, int32_t* idx_out, double* val_out,
                                                   void* stream);

/* Host only: the longest candidate list whose keys a workgroup keeps in local memory for a block of this layout (32-bit
 * keys for f32 and binary16, 64-bit keys for float64); -1 for an unknown layout. */
SIMRANK_CANDIDATES_API int64_t simrank_candidates_staged(int32_t layout);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_CANDIDATES_H */
