/*
 * simrank_diverse.h — diversified selection on the score band of the basket queries (libsimrank_diverse.so).
 *
 * Greedy maximal-marginal-relevance re-ranking of a float64 score band (what simrank_sets_score writes: one row per
 * basket, one column per candidate, -inf = "no candidate") against the matrix S the scores were read from.  Per basket,
 * with rel_w and lam given by the caller (rel_w = 1.0 - lam, formed once on the host):
 *
 *     pen[b] = +0.0 for every candidate b;  live[b] = score[b] is neither NaN nor -inf
 *     repeat k times:
 *         value[b] = (rel_w * score[b]) - (lam * pen[b])     three IEEE double operations, never fused
 *         b* = the live b whose value is not NaN: greatest value first (-0.0 and +0.0 compare equal), then smallest b
 *         none left: stop
 *         emit (b*, score[b*], pen[b*], value[b*]), each with its own bits;  live[b*] = false
 *         for every b:  x = S[row(b*)][col(b)];  if x > pen[b]: pen[b] = x
 *
 * x is widened as simrank_query_rows widens it (f32 -> double; binary16 h -> (float)h * 2^-14 -> double; float64 as it
 * is).  pen starts at +0.0 and only rises: a NaN or negative x never changes it, it is never NaN and never -0.0.  S is in
 * general NOT symmetric: ROW row(b*) is read.  A host loop over NumPy's elementwise `*`, `-` and `np.where(x > pen, x,
 * pen)` reproduces every output bit for bit.
 *
 *     simrank_diverse_pick         S is a block of an iterate, read IN PLACE in one of the four layouts below
 *     simrank_diverse_pick_lists   S is the matrix P of the neighbour tables of simrank_neighbors.h
 *
 * Conventions as simrank_sets.h: 0 or a negative status (SIMRANK_DIVERSE_ERR_*), the message of the last failure on the
 * calling thread from simrank_diverse_last_error(); device pointers are HIP device memory of the current device; `stream`
 * is a hipStream_t passed as void*; every entry point only queues work on it and allocates nothing: the caller passes
 * the workspace that holds the pen vectors.  Argument checks need no device.  Independent of the other headers of this
 * project: this one includes none of them and the library links none of their libraries.
 */
#ifndef SIMRANK_DIVERSE_H
#define SIMRANK_DIVERSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_DIVERSE_VERSION 1
#define SIMRANK_DIVERSE_CHUNK 1024         /* candidates one workgroup visits per turn of a sweep: 256 lanes x 4 */
#define SIMRANK_DIVERSE_MAX_BLOCKS (1 << 24)   /* workgroups of one call: one per basket */

#if defined(__GNUC__)
#define SIMRANK_DIVERSE_API __attribute__((visibility("default")))
#else
#define SIMRANK_DIVERSE_API
#endif

enum {
    SIMRANK_DIVERSE_OK = 0,
    SIMRANK_DIVERSE_ERR_INVALID = -1,  /* bad argument: NULL, shape, layout, k, weights, too many workgroups */
    SIMRANK_DIVERSE_ERR_HIP = -2       /* a HIP runtime call failed */
};

/* layouts of a block of n_rows x n_cols values (`stride` below): simrank_query.h's */
enum {
    SIMRANK_DIVERSE_PANEL_F32 = 0,     /* f32, 32-column panels: (r, c) at ((c >> 5) * stride + r) * 32 + (c & 31) */
    SIMRANK_DIVERSE_ROWMAJOR_F32 = 1,  /* f32 row-major: (r, c) at r * stride + c */
    SIMRANK_DIVERSE_PANEL_F16 = 2,     /* IEEE binary16 holding value x 2^14, 64-column panels:
                                          (r, c) at ((c >> 6) * stride + r) * 64 + (c & 63) */
    SIMRANK_DIVERSE_ROWMAJOR_F64 = 3   /* float64 row-major: (r, c) at r * stride + c */
};

SIMRANK_DIVERSE_API int simrank_diverse_version(void);
SIMRANK_DIVERSE_API const char* simrank_diverse_last_error(void);

/* Workgroups either entry point launches for n_sets baskets of n_out candidates (one per basket); -1 for bad arguments.
 * A caller cuts its baskets into bands so that this stays at or below SIMRANK_DIVERSE_MAX_BLOCKS. */
SIMRANK_DIVERSE_API int64_t simrank_diverse_blocks(int64_t n_sets, int64_t n_out);

/* Bytes of the workspace either entry point needs for n_sets baskets of n_out candidates: room for one pen vector of
 * doubles per basket, each on 16 bytes (f32 and binary16 blocks keep their pens as f32 in it, which is exact for them);
 * -1 for bad arguments.  The workspace is device memory on 8 bytes (on 16 the kernel moves it with 16-byte loads and
 * stores); what it holds before the call does not matter, what it holds after is unspecified. */
SIMRANK_DIVERSE_API int64_t simrank_diverse_workspace_bytes(int64_t n_sets, int64_t n_out);

/* For every basket q < n_sets the procedure above on row q of `band` (device double, n_out values, rows ld_band apart):
 *     idx_out[q * k + t], score_out[q * k + t], pen_out[q * k + t], val_out[q * k + t]     the t-th pick
 * row(b) = row_pos[b] (device int32 [n_out]), or b when row_pos is NULL; col(b) = col_pos[b] (device int32 [n_out]), or b
 * when col_pos is NULL.  A row position outside 0 .. n_rows - 1 or a column position outside 0 .. n_cols - 1 is not read:
 * its x is NaN, which moves no pen.  Slots past the last pick hold id -1 and zeros.  k >= 1; rel_w and lam are finite and
 * lam lies in [0, 1].  The band is read only.  One workgroup per basket makes at most k sweeps of its n_out candidates;
 * a sweep applies the previous pick's row to pen, forms the values and reduces the best in one pass.  Without col_pos a
 * lane takes four consecutive candidates with 16-byte loads of the row (8 bytes of binary16, 2 x 16 of float64), of the
 * band and of pen, where the block, the band and the workspace are aligned for them. */
SIMRANK_DIVERSE_API int simrank_diverse_pick(const void* S, int32_t layout, int64_t stride, int64_t n_rows,
                                             int64_t n_cols, const int32_t* row_pos, const int32_t* col_pos,
                                             int64_t n_out, const double* band, int64_t ld_band, int64_t n_sets,
                                             int32_t k, double rel_w, double lam, int32_t* idx_out, double* score_out,
                                             double* pen_out, double* val_out, void* workspace, void* stream);

/* The same for the matrix P of simrank_neighbors.h's tables (nbr_ids int32 [n][kk], -1 = an empty slot; nbr_vals double
 * [n][kk]; diag double [n]): candidate b is node b, n candidates.  Row b* of P is its list, its diagonal and +0.0
 * everywhere else: the +0.0 moves no pen, the kk entries are applied by scatter (the ids of one row are distinct, as
 * simrank_neighbors_select writes them; an id outside 0 .. n - 1 is an empty slot), and the diagonal meets only pen[b*],
 * which is never read again: diag is not read and may be NULL. */
SIMRANK_DIVERSE_API int simrank_diverse_pick_lists(const int32_t* nbr_ids, const double* nbr_vals, const double* diag,
                                                   int64_t n, int32_t kk, const double* band, int64_t ld_band,
                                                   int64_t n_sets, int32_t k, double rel_w, double lam,
                                                   int32_t* idx_out, double* score_out, double* pen_out,
                                                   double* val_out, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_DIVERSE_H */
