/*
 * simrank_exemplars.h — the two device steps of greedy facility location on a similarity iterate (libsimrank_exemplars.so).
 *
 * Which k rows of a block stand for all its columns?  Greedy facility location picks, k times, the row that raises
 * sum_c max over the picked rows p of S[p][c] the most.  The host keeps the loop; this library computes a row's marginal
 * gain against the running vector of column maxima (`cover`) and applies a picked row to that vector, both on a block
 * of the iterate read IN PLACE.
 *
 * The definitions, all part of the contract.
 *
 *     v(r, c)    the element S[r][c], widened as simrank_query.h's rows widen it (a float, binary16 as (float)h * 2^-14,
 *                a double) and then to double
 *     cover      double [n_cols]; the caller starts it at +0.0 (a column nothing stands for is covered at similarity 0)
 *                and holds no NaN in it
 *     term(r, c) v(r, c) - cover[c] if v(r, c) > cover[c], else +0.0: ONE double subtraction, no fused operation.  The
 *                comparison is false for a NaN element, which therefore never covers, never counts and never gains;
 *                +inf over a finite cover gains +inf
 *     gain(r)    the double sum of term(r, c) over ALL the block's columns (the row's own diagonal element included), in
 *                the order below; NaN when r is outside 0 .. n_rows - 1: no load leaves the block
 *     apply(r)   cover[c] = v(r, c) iff v(r, c) > cover[c], for every column; a row outside the block raises nothing
 *
 * The order of a gain's additions is a function of n_cols alone, the same in all four layouts.  With the terms of the
 * columns at and past n_cols taken as +0.0 (they are not read), T = SIMRANK_EXEMPLARS_THREADS = 256 and the quad
 * q = c / 4 of a column:
 *
 *     1. thread t = q mod T keeps four running sums s_t[0 .. 3]; s_t[i] starts at +0.0 and takes the terms of the
 *        columns 4 (t + T j) + i in the order j = 0, 1, 2, ...
 *     2. x_t = (s_t[0] + s_t[1]) + (s_t[2] + s_t[3])
 *     3. in every wave of 64 consecutive threads an xor butterfly: for d = 32, 16, 8, 4, 2, 1 every lane l replaces its
 *        x by x_l + x_(l xor d); all 64 lanes then hold the same bits w
 *     4. gain = (w_0 + w_1) + (w_2 + w_3) over the four waves
 *
 * Every term is >= +0.0 and every step is a rounded addition in a fixed tree, which is monotone: raising any cover[c]
 * can only lower (or keep) every gain, in floating point as in exact arithmetic.  A gain computed against an older
 * cover is therefore an UPPER BOUND of the gain now, which is what lazy greedy evaluation relies on.  With m the number
 * of columns and E the exact sum of the (rounded) terms: |gain - E| <= (m + 1) * 2^-52 * E.
 *
 * No floating-point atomics anywhere: two runs give the same bits.  `raised` is counted with integer atomics.
 *
 * A block of n_rows x n_cols values is read as the plans of simrank_hip.h report it, in one of the four layouts below.
 *
 * Conventions as simrank_kmedoids.h: 0 or a negative status code (SIMRANK_EXEMPLARS_ERR_*), the message of the last
 * failure on the calling thread from simrank_exemplars_last_error(); device pointers are HIP device memory of the current
 * device; `stream` is a hipStream_t passed as void*; an entry only queues work on it and allocates nothing.  Argument
 * checks need no device.  Independent of the other headers of this project: this one includes none of them and the
 * library links none of their libraries.
 */
#ifndef SIMRANK_EXEMPLARS_H
#define SIMRANK_EXEMPLARS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_EXEMPLARS_VERSION 1
#define SIMRANK_EXEMPLARS_THREADS 256        /* T of the order above: threads of the workgroup that sums one row */
#define SIMRANK_EXEMPLARS_GRID_CAP 2048      /* workgroups of simrank_exemplars_gains at most; more listed rows take turns */

#if defined(__GNUC__)
#define SIMRANK_EXEMPLARS_API __attribute__((visibility("default")))
#else
#define SIMRANK_EXEMPLARS_API
#endif

enum {
    SIMRANK_EXEMPLARS_OK = 0,
    SIMRANK_EXEMPLARS_ERR_INVALID = -1,    /* bad argument: NULL, shape, layout, stride, alignment, n_list */
    SIMRANK_EXEMPLARS_ERR_HIP = -2         /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_EXEMPLARS_PANEL_F32 = 0,       /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_EXEMPLARS_ROWMAJOR_F32 = 1,    /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_EXEMPLARS_PANEL_F16 = 2,       /* IEEE binary16 holding value x 2^14, 64-column panels:
                                              (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_EXEMPLARS_ROWMAJOR_F64 = 3     /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_EXEMPLARS_API int simrank_exemplars_version(void);
SIMRANK_EXEMPLARS_API const char* simrank_exemplars_last_error(void);

/* The gains of listed rows against `cover`, as defined above.  All arrays are device memory.
 *     rows     NULL (the rows 0 .. n_rows - 1; n_list must then be n_rows), or int32 [n_list]: block rows in any order,
 *              repeats allowed; a row outside 0 .. n_rows - 1 gives NaN
 *     cover    const double [n_cols], 8-byte aligned, no NaN
 *     gain     double [n_list]: gain[i] is the gain of block row rows[i]
 * Shapes are below 2^31; element offsets are 64-bit throughout.  A block must start on a multiple of its element's
 * size.  One workgroup of SIMRANK_EXEMPLARS_THREADS threads per listed row, at most SIMRANK_EXEMPLARS_GRID_CAP of them
 * (a workgroup then takes the listed rows i, i + grid, ...); a row is read once, n_list x n_cols elements in all, and
 * `cover` once per listed row (from the L2).  Nothing but `gain` is written.  Asynchronous on `stream`. */
SIMRANK_EXEMPLARS_API int simrank_exemplars_gains(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                                  const int32_t* rows, int64_t n_list, const double* cover, double* gain,
                                                  void* stream);

/* The listed rows applied to `cover` in list order, as defined above.  All arrays are device memory.
 *     rows     int32 [n_list]: block rows; a row outside 0 .. n_rows - 1 raises nothing
 *     cover    double [n_cols], in and out
 *     raised   uint32 [n_list]: raised[i] GROWS by the number of columns whose cover row i raised (integer atomics)
 * A thread owns columns and walks the list, so within a column the rows are applied in the list's order: the result is
 * that of applying them one after the other.  n_list >= 1.  Asynchronous on `stream`. */
SIMRANK_EXEMPLARS_API int simrank_exemplars_cover(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                                  const int32_t* rows, int64_t n_list, double* cover, uint32_t* raised,
                                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_EXEMPLARS_H */
