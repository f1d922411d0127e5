/*
 * simrank_foldin.h — similarities of nodes that were NOT in the fitted graph, from an iterate that stays on the device
 * (libsimrank_foldin.so).
 *
 * A new node q arrives with a neighbour list I_q (fitted nodes) and a row scale w_q.  Its row is what the NEXT update
 * would compute for it with every existing similarity and every existing normalisation held fixed:
 *
 *     s(q, b) = [(1 - lbd)] * E(q, b) * coef * sum_{i in I_q} w_q * sum_{j in I(b)} S[i][j] * scale[b]   [+ lbd * prior(q, b)]
 *     E(q, b) = 1 - 2^-|I_q ∩ I(b)|  over the live rows (w_q > 0, scale[b] > 0), counts saturated at 255
 *
 * for up to SIMRANK_FOLDIN_TILE (32) new nodes at a time, in two stages:
 *
 *     simrank_foldin_gather   T[id(c)][q] = w_q * sum_{i in I_q} S[pos(i)][c]   per column block of the iterate, read IN
 *                             PLACE in one of the four layouts below; T is [n_src][32], one 128-byte (f32) or 256-byte
 *                             (float64) line per source node
 *     simrank_foldin_member   member[j] bit q = (j in I_q and w_q > 0)
 *     simrank_foldin_apply    out[q][b] = epilogue(sum_{j in I(b)} T[j][q], sum_j member[j] bit q), float64 row-major
 *
 * The sums run in f32 for the f32 and binary16 layouts and in float64 for the float64 layout, in a fixed order without
 * floating-point atomics (the same call gives the same bits twice); the epilogue is float64.
 *
 * Conventions as simrank_query.h: 0 or a negative status (SIMRANK_FOLDIN_ERR_*), the message of the last failure on the
 * calling thread from simrank_foldin_last_error(); device pointers are HIP device memory of the current device; `stream`
 * is a hipStream_t passed as void*; every entry point only queues work on it.  A list entry or a CSR column outside its
 * range is not read: it poisons the sums it belongs to with NaN.
 * Independent of the other headers of this project: this one includes none of them and the library links none of their
 * libraries.
 */
#ifndef SIMRANK_FOLDIN_H
#define SIMRANK_FOLDIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_FOLDIN_VERSION 1
#define SIMRANK_FOLDIN_TILE 32         /* new nodes per call: the width of T and of the member word */
#define SIMRANK_FOLDIN_LONG_ROW 256    /* a CSR row with more entries is summed by a whole workgroup (long_rows) */

#if defined(__GNUC__)
#define SIMRANK_FOLDIN_API __attribute__((visibility("default")))
#else
#define SIMRANK_FOLDIN_API
#endif

enum {
    SIMRANK_FOLDIN_OK = 0,
    SIMRANK_FOLDIN_ERR_INVALID = -1,   /* bad argument: NULL, shape, layout, tile width */
    SIMRANK_FOLDIN_ERR_HIP = -2        /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_FOLDIN_PANEL_F32 = 0,      /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_FOLDIN_ROWMAJOR_F32 = 1,   /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_FOLDIN_PANEL_F16 = 2,      /* IEEE binary16 holding value x 2^14, 64-column panels:
                                          (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_FOLDIN_ROWMAJOR_F64 = 3    /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_FOLDIN_API int simrank_foldin_version(void);
SIMRANK_FOLDIN_API const char* simrank_foldin_last_error(void);

/* Bytes of T for n_src source nodes of an iterate in `layout`: n_src x 32 floats (f32 and binary16 layouts) or doubles
 * (float64 layout); -1 for an unknown layout. */
SIMRANK_FOLDIN_API int64_t simrank_foldin_t_bytes(int32_t layout, int64_t n_src);

/* Device memory of the library's own (hipMalloc / hipFree on the current device; 0 bytes gives NULL): what a fold-in
 * holds between its calls (the CSR of a side, T, the member words, the result band) belongs to the kept model and goes
 * back to the driver when the model is released, instead of resting in the main library's block pool. */
SIMRANK_FOLDIN_API int simrank_foldin_alloc(void** ptr, size_t bytes);
SIMRANK_FOLDIN_API int simrank_foldin_free(void* ptr);

/* Stage 1 on one column block: for every column c < n_cols of the block and q < 32,
 *     T[id(c) * 32 + q] = w[q] * sum_{e = list_ptr[q] .. list_ptr[q + 1] - 1} S[list_pos[e]][c]      (0 for q >= n_tile)
 * with id(c) = col_ids[c], or col_base + c when col_ids is NULL (ids outside 0 .. n_src - 1 are not written).
 * list_ptr: device int32 [n_tile + 1] ascending from 0; list_pos: device int32, ROW POSITIONS of the block (the solver's
 * order); w: device double [n_tile].  One workgroup sums 256 (128 in float64) columns for all 32 new nodes with 16-byte
 * (8-byte for binary16) loads along the panel / row, so a source row that several new nodes share comes from HBM once,
 * and writes whole lines of T.  The blocks of one iterate fill disjoint lines of the same T. */
SIMRANK_FOLDIN_API int simrank_foldin_gather(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                                             const int32_t* col_ids, int64_t col_base, const int32_t* list_ptr,
                                             const int32_t* list_pos, const double* w, int32_t n_tile, void* T,
                                             int64_t n_src, void* stream);

/* member[j] (device uint32 [n_src]) = OR over q < n_tile with w[q] > 0 and j in list q of (1 << q); list_ids: device
 * int32, the lists as SOURCE NODE IDS (the ids T is indexed by). */
SIMRANK_FOLDIN_API int simrank_foldin_member(const int32_t* list_ptr, const int32_t* list_ids, const double* w,
                                             int32_t n_tile, uint32_t* member, int64_t n_src, void* stream);

/* Stage 2: for every fitted node b < n_out (CSR rows: rowptr device int32 [n_out + 1], col device int32 source ids,
 * scale device double [n_out]) and q < n_tile
 *     acc = sum_{e in row b} T[col[e]][q]            cnt = sum_e (member[col[e]] >> q) & 1 when scale[b] > 0, else 0
 *     v   = coef * (scale[b] * acc)                                                   member == NULL (no evidence)
 *           (((1 - lbd) * (1 - 2^-min(cnt, 255))) * coef) * (scale[b] * acc)            member != NULL
 *     v  += lbd * prior[q * ld_prior + b]                                             prior != NULL (device double)
 *     out[q * ld_out + b] = v                                          (device double; 256-byte runs per new node)
 * t_layout: the layout of the iterate T was gathered from (it decides T's element type).  long_rows: device int32
 * [n_long], the rows with more than SIMRANK_FOLDIN_LONG_ROW entries, each summed by one workgroup in a fixed order; NULL
 * with n_long = 0 sums every row on half a wave. */
SIMRANK_FOLDIN_API int simrank_foldin_apply(const int32_t* rowptr, const int32_t* col, const double* scale, int64_t n_out,
                                            int64_t n_src, const int32_t* long_rows, int64_t n_long, const void* T,
                                            int32_t t_layout, const uint32_t* member, double coef, double lbd,
                                            const double* prior, int64_t ld_prior, int32_t n_tile, double* out,
                                            int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_FOLDIN_H */
