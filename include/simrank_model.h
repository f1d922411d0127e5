/*
 * simrank_model.h — a kept similarity model as ONE matrix in the caller's order (libsimrank_model.so).
 *
 * A plan of simrank_hip.h holds its iterate in the solver's order, next to the matrices of the loop.  A model that only
 * answers queries needs the iterate alone.  simrank_model_pack copies a block of an iterate — as the plans report it
 * (simrank_plan_get & co: "iterate", "iterate_layout", "iterate_stride", "iterate_rows", "iterate_col_lo",
 * "iterate_col_hi", "ids") or as a float64 row-major matrix — into a destination block the caller owns, rows and
 * columns in the caller's order:
 *
 *     dst[r][col_dst[i]] = src[row_map[r]][col_src[i]]        r < dst_rows, i < n_list
 *
 * The destination is one of the same layouts, so the query, select and fold-in libraries read it as they read a plan's
 * block, with identity orders.  The column blocks of several ranks go into one destination, one call per block.
 *
 * Conventions as simrank_hip.h: 0 or a negative status (SIMRANK_MODEL_ERR_*), the message of the last failure on the
 * calling thread from simrank_model_last_error(); device pointers are HIP device memory of the current device; `stream`
 * is a hipStream_t passed as void*; the entry point only queues work on it and allocates nothing.
 * Independent of the other headers of this project: this one includes none of them and the library links none of their
 * libraries.
 */
#ifndef SIMRANK_MODEL_H
#define SIMRANK_MODEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_MODEL_VERSION 1

#if defined(__GNUC__)
#define SIMRANK_MODEL_API __attribute__((visibility("default")))
#else
#define SIMRANK_MODEL_API
#endif

enum {
    SIMRANK_MODEL_OK = 0,
    SIMRANK_MODEL_ERR_INVALID = -1,    /* bad argument: NULL, shape, layout, a pair of layouts that is not packed */
    SIMRANK_MODEL_ERR_HIP = -2         /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_MODEL_PANEL_F32 = 0,       /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31); stride = rows_pad */
    SIMRANK_MODEL_ROWMAJOR_F32 = 1,    /* f32 row-major: (r, c) at r * stride + c; stride = ld */
    SIMRANK_MODEL_PANEL_F16 = 2,       /* IEEE binary16 holding value x 2^14, 64-column panels:
                                          (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63); stride = rows_pad */
    SIMRANK_MODEL_ROWMAJOR_F64 = 3     /* float64 row-major: (r, c) at r * stride + c; stride = ld */
};

SIMRANK_MODEL_API int simrank_model_version(void);
SIMRANK_MODEL_API const char* simrank_model_last_error(void);

/* dst[r][col_dst[i]] = src[row_map[r]][col_src[i]] for r < dst_rows, i < n_list.
 *   src         block of src_rows x src_cols values in src_layout / src_stride
 *   row_map     device int32 [dst_rows]: destination row -> source row; NULL = the same row (dst_rows <= src_rows)
 *   col_dst     device int32 [n_list]: destination columns, best ascending; NULL = 0 .. n_list - 1 (n_list <= dst_cols)
 *   col_src     device int32 [n_list]: their source columns within the block; NULL = 0 .. n_list - 1 (n_list <= src_cols)
 *   dst         block of dst_rows x dst_cols values in dst_layout / dst_stride, 16-byte aligned
 * An entry of a map that points outside its block is skipped: nothing is read and nothing written for it.
 *
 * Pairs of layouts: PANEL_F32 or ROWMAJOR_F32 -> ROWMAJOR_F32, PANEL_F16 -> PANEL_F16, ROWMAJOR_F64 -> ROWMAJOR_F64 move
 * the bits unchanged (`overflow` is not used).  PANEL_F32 or ROWMAJOR_F32 -> PANEL_F16 converts: the stored binary16 is
 * x * 2^14 rounded to nearest even, and the number of elements whose stored value is not finite (an overflow, or a source
 * that was not finite) is ADDED to *overflow (device int64, required; zero it first).  Every other pair is refused.
 *
 * One 256-thread workgroup writes a run of consecutive destination entries of one destination row, 16 bytes per lane
 * where col_dst is NULL and the destination's rows are 16-byte aligned (a row-major stride that is a multiple of 16
 * bytes; panels always), and gathers their sources from one source row; the workgroups of a destination row share
 * blockIdx % 8, so that the source row is fetched into one L2.  Offsets are 64-bit; the rows are cut into bands so that
 * no launch reaches 2^32 work-items.  n_list < 2^29. */
SIMRANK_MODEL_API int simrank_model_pack(const void* src, int32_t src_layout, int64_t src_stride, int64_t src_rows,
                                         int64_t src_cols, const int32_t* row_map, const int32_t* col_dst,
                                         const int32_t* col_src, int64_t n_list, void* dst, int32_t dst_layout,
                                         int64_t dst_stride, int64_t dst_rows, int64_t dst_cols, int64_t* overflow,
                                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_MODEL_H */
