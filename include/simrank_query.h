/*
 * simrank_query.h — node queries on a similarity iterate that stays on the device (libsimrank_query.so).
 *
 * "What is similar to THESE nodes?" and "how similar are a and b?" after one fit, without handing the dense N x N matrix
 * back: chosen rows, chosen pairs and the k best of chosen rows are read out of a block of the iterate IN PLACE, as the
 * plans of simrank_hip.h hold it (simrank_plan_get / simrank_biplan_get / simrank_shardplan_get, keys "iterate",
 * "iterate_layout", "iterate_stride", "iterate_rows", "iterate_col_lo", "iterate_col_hi", "ids") or as a float64
 * row-major matrix:
 *
 *     simrank_query_rows(S, ..., row_pos, n_q, col_pos, n_out, out, ld_out)    out[q][j] = (double)S[row_pos[q]][col_pos[j]]
 *     simrank_query_pairs(S, ..., a_pos, b_pos, n_pairs, out)                  out[i]    = (double)S[a_pos[i]][b_pos[i]]
 *     simrank_query_topk(S, ..., row_pos, row_ids, n_q, col_ids, k, idx, val)  the k largest of each chosen row
 *
 * Positions are rows / columns of the BLOCK (the solver's order); the caller turns node ids into positions by inverting
 * the plan's "ids" once.  Every value is widened to double on the device exactly as the dense hand-back widens it
 * (f32 -> double exact; binary16 h -> (float)h * 2^-14 -> double; float64 copied), so a queried value is bit-identical to
 * the same element of the dense result.
 *
 * Conventions as simrank_hip.h: 0 or a negative status (SIMRANK_QUERY_ERR_*), the message of the last failure on the
 * calling thread from simrank_query_last_error(); device pointers are HIP device memory of the current device; `stream`
 * is a hipStream_t passed as void*; every entry point only queues work on it.  A position outside the block is not read:
 * its value is reported as NaN (rows / pairs) or its row as empty (top-k).
 * Independent of the other headers of this project: this one includes none of them and the library links none of their
 * libraries.
 */
#ifndef SIMRANK_QUERY_H
#define SIMRANK_QUERY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_QUERY_VERSION 1

#if defined(__GNUC__)
#define SIMRANK_QUERY_API __attribute__((visibility("default")))
#else
#define SIMRANK_QUERY_API
#endif

enum {
    SIMRANK_QUERY_OK = 0,
    SIMRANK_QUERY_ERR_INVALID = -1,    /* bad argument: NULL, shape, layout, k */
    SIMRANK_QUERY_ERR_HIP = -2         /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below); 0 .. 2 are simrank_select.h's */
enum {
    SIMRANK_QUERY_PANEL_F32 = 0,       /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31); stride = rows_pad */
    SIMRANK_QUERY_ROWMAJOR_F32 = 1,    /* f32 row-major: (r, c) at r * stride + c; stride = ld */
    SIMRANK_QUERY_PANEL_F16 = 2,       /* IEEE binary16 holding value x 2^14, 64-column panels:
                                          (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63); stride = rows_pad */
    SIMRANK_QUERY_ROWMAJOR_F64 = 3     /* float64 row-major: (r, c) at r * stride + c; stride = ld */
};

SIMRANK_QUERY_API int simrank_query_version(void);
SIMRANK_QUERY_API const char* simrank_query_last_error(void);

/* out[q * ld_out + j] (device, double) = S[row_pos[q]][col_pos[j]] for q < n_q, j < n_out.  row_pos: device int32 [n_q];
 * col_pos: device int32 [n_out], or NULL for the columns 0 .. n_out - 1 themselves (n_out <= n_cols).  ld_out >= n_out.
 * One workgroup writes 1024 consecutive doubles of one query row (coalesced 8-byte stores) and gathers their sources
 * from the row's segments; the workgroups of one query row share blockIdx % 8, so that the row is fetched into one L2. */
SIMRANK_QUERY_API int simrank_query_rows(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                         const int32_t* row_pos, int64_t n_q, const int32_t* col_pos, int64_t n_out,
                                         double* out, int64_t ld_out, void* stream);

/* out[i] (device, double) = S[a_pos[i]][b_pos[i]] for i < n_pairs (device int32 arrays). */
SIMRANK_QUERY_API int simrank_query_pairs(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                          const int32_t* a_pos, const int32_t* b_pos, int64_t n_pairs, double* out,
                                          void* stream);

/* For q < n_q: the k largest entries of row row_pos[q] among the columns c with col_ids[c] != row_ids[q] (the row's own
 * node is excluded BY ID, so the rows may be any subset in any order and the block any column range), in the total order
 * (value descending, id ascending).  idx_out[q * k + j] (device int32) = col_ids[c] of the j-th, val_out[q * k + j]
 * (device double) its value; slots past the number of candidates hold id -1 and value 0.  row_ids: device int32 [n_q];
 * col_ids: device int32 [n_cols], or NULL for the positions 0, 1, ....  1 <= k <= 1024.  One wave per query row, which
 * sweeps the row once per pick: k x n_cols reads per query row (from L2 after the first sweep), so the cost grows with k
 * — right for the tens of neighbours a query asks for, slow for k in the hundreds over many rows. */
SIMRANK_QUERY_API int simrank_query_topk(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                         const int32_t* row_pos, const int32_t* row_ids, int64_t n_q,
                                         const int32_t* col_ids, int32_t k, int32_t* idx_out, double* val_out,
                                         void* stream);

/* Host only: n_pieces candidate lists for the SAME n_q query rows (piece p: ids[p] int32 [n_q * ks[p]], vals[p] double
 * [n_q * ks[p]], as simrank_query_topk wrote them for one column block each; id -1 = empty slot) into the k best per
 * row in the same total order; slots past the number of candidates hold id -1 and value 0. */
SIMRANK_QUERY_API int simrank_query_merge_topk(int32_t n_pieces, const int32_t* const* ids, const double* const* vals,
                                               const int32_t* ks, int64_t n_q, int32_t k, int32_t* idx_out,
                                               double* val_out);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_QUERY_H */
