/*
 * simrank_select.h — result queries on a similarity iterate that stays on the device (libsimrank_select.so).
 *
 * "Which pairs of nodes are at least t similar?" without handing the dense N x N matrix back: a COUNT pass and an EMIT
 * pass over a block of the iterate as the plans of simrank_hip.h hold it (simrank_plan_get / simrank_biplan_get /
 * simrank_shardplan_get, keys "iterate", "iterate_layout", "iterate_stride", "iterate_rows", "iterate_col_lo",
 * "iterate_col_hi", "ids"), then the hits into the caller's order on the host:
 *
 *     simrank_select_threshold_f32(t, &t32)                          once, on the host
 *     simrank_select_count(S, ..., t32, counts_dev, stream)          per row: #{c : S[r][c] >= t32, id(c) != id(r)}
 *     simrank_select_offsets(counts_host, n, offsets_host, &total)   exclusive scan into int64 (total may pass 2^31)
 *     simrank_select_emit(S, ..., t32, offsets_dev, total, ...)      (caller id, value) of every hit, rows in the
 *                                                                     block's order, columns ascending in it
 *     simrank_select_merge(pieces, ..., row_order, ...)              rows into the caller's order, each row's
 *                                                                     neighbours ascending by caller id
 *
 * A pair is a hit iff (double)S[r][c] >= t: simrank_select_threshold_f32 gives the smallest float t32 with
 * (double)t32 >= t, and the kernels compare in f32 (exactly the same set).  fp16-held values are read in place; a value
 * is reported as (float)h * 2^-14, bit-identical to what the dense hand-back widens.
 *
 * Conventions as simrank_hip.h: 0 or a negative status (SIMRANK_SELECT_ERR_*), the message of the last failure on the
 * calling thread from simrank_select_last_error(); device pointers are HIP device memory of the current device (the
 * main library's simrank_malloc is the intended allocator of scratch); `stream` is a hipStream_t passed as void*.
 * Independent of simrank_hip.h: this header includes nothing of it and the library links nothing of it.
 */
#ifndef SIMRANK_SELECT_H
#define SIMRANK_SELECT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_SELECT_VERSION 1

#if defined(__GNUC__)
#define SIMRANK_SELECT_API __attribute__((visibility("default")))
#else
#define SIMRANK_SELECT_API
#endif

enum {
    SIMRANK_SELECT_OK = 0,
    SIMRANK_SELECT_ERR_INVALID = -1,   /* bad argument: NULL, shape, layout, threshold, order */
    SIMRANK_SELECT_ERR_HIP = -2        /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below) */
enum {
    SIMRANK_SELECT_PANEL_F32 = 0,      /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31); stride = rows_pad */
    SIMRANK_SELECT_ROWMAJOR_F32 = 1,   /* f32 row-major: (r, c) at r * stride + c; stride = ld */
    SIMRANK_SELECT_PANEL_F16 = 2       /* IEEE binary16 holding value x 2^14, 64-column panels:
                                          (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63); stride = rows_pad */
};

SIMRANK_SELECT_API int simrank_select_version(void);
SIMRANK_SELECT_API const char* simrank_select_last_error(void);

/* the smallest float t32 with (double)t32 >= t; t must be finite and > 0.  Host only, no device. */
SIMRANK_SELECT_API int simrank_select_threshold_f32(double t, float* t32);

/* counts[r] (device, int32, n_rows) = number of columns c of row r with S[r][c] >= t32 and col_ids[c] != row_ids[r].
 * row_ids / col_ids: device int32 arrays of the rows' and the columns' node ids (NULL = the positions 0, 1, ...).
 * A wave takes eight rows of a panel layout (16-byte loads, the eight rows' segments of a panel contiguous) or one row
 * of the row-major layout.  Asynchronous on `stream`. */
SIMRANK_SELECT_API int simrank_select_count(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                            const int32_t* row_ids, const int32_t* col_ids, float t32, int32_t* counts,
                                            void* stream);

/* offsets[0] = 0, offsets[r + 1] = offsets[r] + counts[r] (host arrays: n_rows counts, n_rows + 1 offsets); *total =
 * offsets[n_rows].  Host only. */
SIMRANK_SELECT_API int simrank_select_offsets(const int32_t* counts, int64_t n_rows, int64_t* offsets, int64_t* total);

/* The same rows and test as simrank_select_count: hit j of row r (columns ascending) goes to slot offsets[r] + j of
 * ids_out (col_ids[c], int32) and vals_out (the value, f32).  offsets: device int64 [n_rows + 1].  Nothing is written at
 * or past offsets[r + 1] nor at or past `capacity` (the length of both output arrays).  The slot of a hit is decided by
 * ballots and prefix counts inside the wave: no atomics, the same output on every run.  Asynchronous on `stream`. */
SIMRANK_SELECT_API int simrank_select_emit(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                           const int32_t* row_ids, const int32_t* col_ids, float t32,
                                           const int64_t* offsets, int64_t capacity, int32_t* ids_out, float* vals_out,
                                           void* stream);

/* Host: n_pieces blocks of hits over the SAME n_rows rows (piece p: offsets[p] [n_rows + 1], ids[p], vals[p], as
 * simrank_select_emit wrote them — one piece per column block of a sharded iterate) into the caller's order: row r of
 * the pieces is the caller's row row_order[r] (a permutation of 0 .. n_rows - 1); out_offsets [n_rows + 1] is indexed by
 * caller row, and each row's hits are concatenated over the pieces and sorted ascending by id (ids in a row must be
 * distinct).  out_ids / out_vals hold the sum of the pieces' totals.  On up to `threads` host threads (<= 0: automatic),
 * never more than 16 nor more than the process may use. */
SIMRANK_SELECT_API int simrank_select_merge(int32_t n_pieces, const int64_t* const* offsets, const int32_t* const* ids,
                                            const float* const* vals, int64_t n_rows, const int32_t* row_order,
                                            int64_t* out_offsets, int32_t* out_ids, float* out_vals, int32_t threads);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_SELECT_H */
