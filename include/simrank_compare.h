/*
 * simrank_compare.h — how far apart two similarity iterates are, measured where they lie (libsimrank_compare.so).
 *
 * Two blocks A and B over the SAME rows and columns in the SAME order, each in any of the four layouts below, are swept
 * once IN PLACE.  Per row a few numbers come back, over the whole block an exponent histogram.  Every statistic is a
 * maximum or an integer count: nothing is a floating-point sum, so every output is a function of the two blocks alone
 * and two runs (or a restatement in NumPy) give the same bits.
 *
 * The definitions, all part of the contract.  For a pair of elements a = A[r][c], b = B[r][c], each widened as
 * simrank_query.h's rows widen it (a float to double; binary16 as (float)h * 2^-14, then to double; a double as it is):
 *
 *     d      +0.0 if a == b (so -0.0 and +0.0 agree, and equal infinities agree) or if both are NaN;
 *            +inf if exactly one of them is NaN;
 *            otherwise fabs(a - b), one subtraction in double.  d is never NaN.
 *     rel    the first rule that applies, in this order:
 *            +0.0 if d == 0 or max(|a|, |b|) < floor (a NaN operand makes that maximum NaN, which is below nothing; two
 *            finite values below the floor whose difference overflows to +inf are still +0.0);
 *            +inf if d == inf;
 *            otherwise d / max(|a|, |b|), one correctly rounded division.
 *
 * Per row r, the diagonal included:
 *
 *     max_abs[r]    the largest d;  arg_abs[r] the smallest column attaining it.  An empty row (n_cols == 0): 0.0 and -1.
 *     max_rel[r]    the largest rel; arg_rel[r] the smallest column attaining it, as above.
 *     over[r][t]    the number of columns with d > tol[t] (uint32), for n_tol <= SIMRANK_COMPARE_MAX_TOL tolerances.
 *
 * Over the whole block, hist[bits(d) >> 52] += 1 for every element: bin 0 holds d == 0 and subnormal d, bin e the d with
 * 2^(e-1023) <= d < 2^(e-1022), bin 2047 holds d == inf.  hist is ADDED to: that is how a caller sums over pieces.
 *
 * No load leaves either block; the padding columns of a panel are never counted.
 *
 * Conventions as simrank_groups.h: 0 or a negative status code (SIMRANK_COMPARE_ERR_*), the message of the last failure
 * on the calling thread from simrank_compare_last_error(); device pointers are HIP device memory of the current device;
 * `stream` is a hipStream_t passed as void*; the entry only queues work on it and allocates nothing.  Argument checks
 * need no device.  Independent of the other headers of this project: this one includes none of them and the library
 * links none of their libraries.
 */
#ifndef SIMRANK_COMPARE_H
#define SIMRANK_COMPARE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_COMPARE_VERSION 1
#define SIMRANK_COMPARE_MAX_TOL 8           /* tolerances of one sweep */
#define SIMRANK_COMPARE_BINS 2048           /* exponent bins of the histogram */
#define SIMRANK_COMPARE_MAX_GRID 2048       /* workgroups of one sweep, four waves each, a wave a row at a time */

#if defined(__GNUC__)
#define SIMRANK_COMPARE_API __attribute__((visibility("default")))
#else
#define SIMRANK_COMPARE_API
#endif

enum {
    SIMRANK_COMPARE_OK = 0,
    SIMRANK_COMPARE_ERR_INVALID = -1,      /* bad argument: NULL, shape, layout, stride, tolerances */
    SIMRANK_COMPARE_ERR_HIP = -2           /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride_a`, `stride_b` below): simrank_query.h's */
enum {
    SIMRANK_COMPARE_PANEL_F32 = 0,         /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_COMPARE_ROWMAJOR_F32 = 1,      /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_COMPARE_PANEL_F16 = 2,         /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_COMPARE_ROWMAJOR_F64 = 3       /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_COMPARE_API int simrank_compare_version(void);
SIMRANK_COMPARE_API const char* simrank_compare_last_error(void);

/* One sweep of the two blocks, as defined above.
 *     A, B       device memory: the two blocks, each in its own layout and stride, any of the 16 pairs.  A block must
 *                start on a multiple of its element's size; where every quad of four columns is one aligned vector
 *                load (a panel block on 16 bytes, 8 for binary16; a row-major block whose rows start on 16 bytes) the
 *                side is read with vector loads, otherwise element by element
 *     tol        HOST memory, double [n_tol], read before the call returns: finite and >= 0; NULL iff n_tol == 0
 *     floor      finite and >= 0
 *     max_abs, max_rel   device double [n_rows];  arg_abs, arg_rel  device int32 [n_rows]
 *     over       device uint32 [n_rows][n_tol]; NULL iff n_tol == 0
 *     hist       device unsigned 64-bit [SIMRANK_COMPARE_BINS], added to with integer atomics
 * Shapes are below 2^31; element offsets are 64-bit throughout.  A workgroup counts in 32-bit bins: a call that would
 * give one workgroup 2^32 elements or more (min(n_rows, 4 * ceil(n_rows / (4 * SIMRANK_COMPARE_MAX_GRID))) * n_cols) is
 * refused; sweep such a block in bands of fewer rows.  Nothing but the outputs is written.  Asynchronous on `stream`. */
SIMRANK_COMPARE_API int simrank_compare_sweep(const void* A, int32_t layout_a, int64_t stride_a, const void* B,
                                              int32_t layout_b, int64_t stride_b, int64_t n_rows, int64_t n_cols,
                                              const double* tol, int32_t n_tol, double floor, double* max_abs,
                                              int32_t* arg_abs, double* max_rel, int32_t* arg_rel, uint32_t* over,
                                              unsigned long long* hist, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_COMPARE_H */
