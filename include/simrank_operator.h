/*
 * simrank_operator.h — a kept model as a linear operator (libsimrank_operator.so).
 *
 * The product of the matrix S of a kept model with a dense block of at most SIMRANK_OPERATOR_MAX_D column vectors, S
 * read IN PLACE from a block of the iterate in one of the four layouts below:
 *
 *     transpose = 0     out[a][q] = alpha * sum_b S[row(a)][col(b)] * X[b][q] + beta * out[a][q]     a < n_rows, b < n_cols
 *     transpose = 1     out[b][q] = alpha * sum_a S[row(a)][col(b)] * X[a][q] + beta * out[b][q]     b < n_cols, a < n_rows
 *
 * for q < d.  Every element of S is widened as simrank_query_rows widens it (f32 -> double; binary16 h -> (float)h *
 * 2^-14 -> double; float64 as it is); products and sums are IEEE doubles and may be fused multiply-adds.  The order of
 * a sum's additions is a function of n_rows, n_cols, transpose and d alone and no floating-point atomic is used: the
 * same call gives the same bits twice, and a sum of K terms lies within K * 2^-52 * sum |S| |X| of the exact one.  With
 * beta == 0 `out` is not read: whatever it held, NaN included, is overwritten.
 *
 * Conventions as simrank_query.h: 0 or a negative status (SIMRANK_OPERATOR_ERR_*), the message of the last failure on
 * the calling thread from simrank_operator_last_error(); device pointers are HIP device memory of the current device;
 * `stream` is a hipStream_t passed as void*; the entry point only queues work on it and allocates nothing: the caller
 * passes the workspace.  Argument checks need no device.  Independent of the other headers of this project: this one
 * includes none of them and the library links none of their libraries.
 */
#ifndef SIMRANK_OPERATOR_H
#define SIMRANK_OPERATOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_OPERATOR_VERSION 1
#define SIMRANK_OPERATOR_MAX_D 64          /* columns of X in one call: a caller cuts a wider X into bands */
#define SIMRANK_OPERATOR_NARROW 8          /* d up to here takes the matrix-vector forms, which keep S in registers */
#define SIMRANK_OPERATOR_STRIP 128         /* output rows of one workgroup for a wider X */
#define SIMRANK_OPERATOR_MAX_PARTS 64      /* parts the contraction is cut into at most */

#if defined(__GNUC__)
#define SIMRANK_OPERATOR_API __attribute__((visibility("default")))
#else
#define SIMRANK_OPERATOR_API
#endif

enum {
    SIMRANK_OPERATOR_OK = 0,
    SIMRANK_OPERATOR_ERR_INVALID = -1,  /* bad argument: NULL, shape, layout, d, leading dimension, transpose */
    SIMRANK_OPERATOR_ERR_HIP = -2       /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_OPERATOR_PANEL_F32 = 0,     /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_OPERATOR_ROWMAJOR_F32 = 1,  /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_OPERATOR_PANEL_F16 = 2,     /* IEEE binary16 holding value x 2^14, 64-column panels:
                                           (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_OPERATOR_ROWMAJOR_F64 = 3   /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_OPERATOR_API int simrank_operator_version(void);
SIMRANK_OPERATOR_API const char* simrank_operator_last_error(void);

/* Parts the contraction of a call of this shape is cut into (1 .. SIMRANK_OPERATOR_MAX_PARTS): a function of the shape,
 * the direction and d alone, so that a small matrix still fills the device; every part's partial sums are written to the
 * workspace and added in the order of the parts.  -1 for bad arguments. */
SIMRANK_OPERATOR_API int64_t simrank_operator_parts(int64_t n_rows, int64_t n_cols, int32_t transpose, int32_t d);

/* Bytes of the workspace simrank_operator_apply needs for this shape: parts x output rows x d doubles (at least 8);
 * -1 for bad arguments.  Device memory on 8 bytes; what it holds before the call does not matter, what it holds after
 * is unspecified. */
SIMRANK_OPERATOR_API int64_t simrank_operator_workspace_bytes(int64_t n_rows, int64_t n_cols, int32_t transpose,
                                                              int32_t d);

/* The product above.  X (device double, row-major, rows ld_x apart, ld_x >= d) has n_cols rows for transpose = 0 and
 * n_rows for transpose = 1; out (device double, rows ld_out apart, ld_out >= d) has n_rows and n_cols.  X and out must
 * not overlap.  1 <= d <= SIMRANK_OPERATOR_MAX_D.
 * row(a) = row_pos[a] (device int32 [n_rows]), or a when row_pos is NULL; col(b) = col_pos[b] (device int32 [n_cols]),
 * or b when col_pos is NULL.  A row position outside 0 .. n_rows - 1 or a column position outside 0 .. n_cols - 1 is
 * not read: its elements are NaN and poison the sums they belong to.
 * One workgroup takes SIMRANK_OPERATOR_STRIP output rows (a row strip of S, or a column strip for transpose = 1) and
 * one part of the contraction; tiles of S and X go through local memory.  For d <= SIMRANK_OPERATOR_NARROW a workgroup
 * takes 16 rows of S (transpose = 0: four per wave, a row's partial sums added across the wave's lanes) or 1024 columns
 * (transpose = 1: four per lane) and keeps its elements of S in registers; only the tiles of X go through local memory.
 * Without col_pos, S is read with 16-byte loads (8 bytes of binary16, 2 x 16 of float64) where the block is aligned for
 * them: panels on 16 (8) bytes, row-major rows on 16 bytes; element by element otherwise. */
SIMRANK_OPERATOR_API int simrank_operator_apply(const void* S, int32_t layout, int64_t stride, int64_t n_rows,
                                                int64_t n_cols, const int32_t* row_pos, const int32_t* col_pos,
                                                int32_t transpose, const double* X, int64_t ld_x, int32_t d,
                                                double alpha, double beta, double* out, int64_t ld_out,
                                                void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_OPERATOR_H */
