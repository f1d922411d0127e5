/*
 * simrank_f64.h — the reference's float64 loop on one GPU (libsimrank_f64.so).
 *
 * Every class's update is  X' = C . W Y W^T  (then optionally .* E and (1 - lbd) . + lbd . A), then diag(X') = 1, with
 * W = diag(rowscale) . P and P the 0/1 pattern of a CSR graph (SimRank.py:139, :361, :453; the bipartite classes run
 * two such updates per loop index, the second reading the first's new matrix, :298-301).  A plan holds one side (a
 * square pattern) or two (an n1 x n2 pattern and its n2 x n1 transpose) and runs each update as two gather legs in
 * float64, caller's node order kept:
 *
 *     leg A   T = W . Y by gathering rows of Y, stored transposed (16 x 16 tiles through LDS)
 *     leg B   rows of W . T^T = (W Y W^T)^T by gathering rows of T^T, the epilogue (C, 1 - 0.5^count, the prior blend,
 *             diag = 1) and the count of |new - old| > eps fused in.  Symmetric iterates (options.symmetric): the upper
 *             triangle only, then a mirror pass; otherwise the whole product, then a tiled transpose pass that applies
 *             the epilogue in place.
 *
 *     simrank_f64_plan_create(sides, n_sides, &options, stream, &plan)   S = I on every side
 *     simrank_f64_plan_step(plan, eps, changed)                          one loop index's update(s) + their counts
 *     simrank_f64_plan_result / _topk / _count_above + _emit_above       hand-backs of side `side` (0 or 1)
 *     simrank_f64_plan_trim / _destroy
 *
 * The loop itself (the convergence test at loop index 0, iterations = 0, eps >= 1, the progress hook per loop index)
 * is the caller's: one step per loop index, read the counts.
 *
 * Conventions: 0 or a negative status (SIMRANK_F64_ERR_*), the message of the last failure on the calling thread from
 * simrank_f64_last_error(); `stream` is a hipStream_t passed as void*; the plan owns the device memory it allocates and
 * checks the free device memory before it allocates.  The evidence counts are the caller's device memory (u8, as the
 * main library's simrank_evidence_counts writes them); they must stay alive as long as the plan.  Independent of
 * simrank_hip.h: this header includes nothing of it and the library links nothing of it.
 */
#ifndef SIMRANK_F64_H
#define SIMRANK_F64_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_F64_VERSION 1

#if defined(__GNUC__)
#define SIMRANK_F64_API __attribute__((visibility("default")))
#else
#define SIMRANK_F64_API
#endif

enum {
    SIMRANK_F64_OK = 0,
    SIMRANK_F64_ERR_INVALID = -1,      /* bad argument: NULL, shape, side, released matrices */
    SIMRANK_F64_ERR_HIP = -2,          /* a HIP runtime call failed */
    SIMRANK_F64_ERR_MEMORY = -3        /* not enough free device memory for the plan */
};

typedef struct simrank_f64_plan simrank_f64_plan;

/* One similarity matrix of a fit: W = diag(rowscale) . P with P an n_rows x n_cols pattern (CSR, host arrays, copied;
 * column indices in [0, n_cols)).  The matrix is n_rows x n_rows. */
typedef struct simrank_f64_side {
    int64_t n_rows, n_cols, nnz;
    const int32_t* rowptr;             /* host, n_rows + 1 */
    const int32_t* col;                /* host, nnz (NULL when nnz = 0) */
    const double* rowscale;            /* host, n_rows */
    double coef;                       /* C */
    const uint8_t* counts;             /* DEVICE u8 common in-neighbour counts, row-major; NULL = no evidence factor */
    int64_t counts_ld;                 /* row pitch of counts, bytes */
    int64_t counts_n;                  /* counts is counts_n x counts_n: n_rows, or 1 (one count for every pair) */
    const double* prior;               /* host float64 n_rows x n_rows row-major, copied; NULL = no prior */
    double lbd;                        /* weight of the prior */
} simrank_f64_side;

typedef struct simrank_f64_options {
    int32_t symmetric;                 /* 1: every iterate is symmetric (no prior, or symmetric priors): upper triangle +
                                          mirror; 0: the whole product (any prior) */
} simrank_f64_options;

SIMRANK_F64_API int simrank_f64_version(void);
SIMRANK_F64_API const char* simrank_f64_last_error(void);

/* Device bytes a plan of these sides allocates (the check plan_create makes against the free memory).  Host only. */
SIMRANK_F64_API int simrank_f64_plan_bytes(const simrank_f64_side* sides, int32_t n_sides, int64_t* bytes);
/* Free and total memory of the current device (hipMemGetInfo). */
SIMRANK_F64_API int simrank_f64_mem_info(int64_t* free_bytes, int64_t* total_bytes);

/* n_sides = 1: sides[0] square (n_rows = n_cols).  n_sides = 2: sides[1]'s pattern is the transpose of sides[0]'s
 * (n_rows / n_cols swapped, the same nnz).  Update of side 0 reads the matrix of side 1 (two sides) or its own. */
SIMRANK_F64_API int simrank_f64_plan_create(const simrank_f64_side* sides, int32_t n_sides,
                                            const simrank_f64_options* options, void* stream, simrank_f64_plan** out);
SIMRANK_F64_API int simrank_f64_plan_destroy(simrank_f64_plan* p);
/* every side's matrix back to I */
SIMRANK_F64_API int simrank_f64_plan_reset(simrank_f64_plan* p);
/* One loop index: side 0's update, then side 1's (reading side 0's new matrix).  changed[s] (host, n_sides entries) =
 * number of elements of side s with |new - old| > eps, compared in float64.  Synchronises the stream. */
SIMRANK_F64_API int simrank_f64_plan_step(simrank_f64_plan* p, double eps, int64_t* changed);
/* HIP-event timing of the next steps: on != 0 starts (and zeroes) the sums; ms[3] = leg A, leg B, mirror / epilogue
 * pass summed over the steps since, and *steps their number. */
SIMRANK_F64_API int simrank_f64_plan_set_timing(simrank_f64_plan* p, int32_t on);
SIMRANK_F64_API int simrank_f64_plan_leg_times(simrank_f64_plan* p, double* ms, int32_t* steps);

/* HOST float64 n x n of side `side`, rows ld doubles apart (ld >= n). */
SIMRANK_F64_API int simrank_f64_plan_result(simrank_f64_plan* p, int32_t side, double* dst, int64_t ld);
/* The k most similar OTHER nodes of every node (exclude_diag = 1) or of every node and itself (0): HOST int32 / double
 * [n][k], largest first, ties by the lower id, -1 / 0 where a row has fewer than k.  1 <= k <= n. */
SIMRANK_F64_API int simrank_f64_plan_topk(simrank_f64_plan* p, int32_t side, int32_t k, int32_t exclude_diag,
                                          int32_t* idx_host, double* val_host);
/* Pairs of DIFFERENT nodes with S[r][c] >= t (float64 comparison; t finite and > 0): offsets_host [n + 1] (host int64)
 * = the exclusive scan of the per-row counts.  Leaves the counts on the device for _emit_above with the same t. */
SIMRANK_F64_API int simrank_f64_plan_count_above(simrank_f64_plan* p, int32_t side, double t, int64_t* offsets_host);
/* The hits of _count_above (same side and t): row r's neighbours ascending at ids_host / vals_host [offsets[r] ..
 * offsets[r + 1]), both of length total = offsets[n].  Slots come from ballots and prefix counts inside a wave: no
 * atomics, one deterministic output. */
SIMRANK_F64_API int simrank_f64_plan_emit_above(simrank_f64_plan* p, int32_t side, double t, int64_t total,
                                                int32_t* ids_host, double* vals_host);
/* Release the matrices (result, topk and the selection fail afterwards). */
SIMRANK_F64_API int simrank_f64_plan_trim(simrank_f64_plan* p);
/* Where side `side`'s CURRENT matrix is, for a reader that works on it in place (include/simrank_query.h, layout
 * float64 row-major): "iterate" the device address (0 after simrank_f64_plan_trim; it moves with every step, so ask
 * after the loop), "iterate_ld" its pitch in doubles, "iterate_rows" n.  Rows and columns are in the caller's order.
 * SIMRANK_F64_ERR_INVALID for a NULL argument, a side out of range or an unknown key. */
SIMRANK_F64_API int simrank_f64_plan_get(const simrank_f64_plan* p, int32_t side, const char* key, int64_t* value);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_F64_H */
