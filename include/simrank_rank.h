/*
 * simrank_rank.h — held-out ranks on a score band that stays on the device (libsimrank_rank.so).
 *
 * The band is the float64 row-major band simrank_sets_score and simrank_neighbors_score write: n_sets rows (one per
 * basket) of n_out values, ld_band apart, -inf where a column is excluded.  A basket lists TARGETS, columns whose place
 * in the basket's ranking is asked for.  The rank of a target is one integer: the number of candidates that precede it in
 * the total order of simrank_sets_topk (score descending, id ascending), plus one.  It is counted here, where the band
 * lies; the band never crosses to the host.
 *
 *     simrank_rank_gather   the band's value at every target whose column lies in this block
 *     simrank_rank_count    per target the candidates of this block that precede it, per basket the block's candidates,
 *                           both ADDED to the caller's counters: a model in several column blocks sums over its blocks
 *
 * The targets of all baskets come as CSR-like device arrays over one numbering x of targets:
 *     tgt_ptr    int64 [n_sets + 1], ascending: basket q's targets are x = tgt_ptr[q] .. tgt_ptr[q + 1] - 1
 *     tgt_col    int32, per target its column within this block, or -1 where its column is not in this block
 *     tgt_id     int32, per target its id in the tie order
 *     tgt_score  double, per target its score: written by gather, read by count
 * A caller that cuts its baskets into bands passes tgt_ptr + first basket and the per-target arrays whole, as
 * simrank_sets_score takes set_ptr.
 *
 * Conventions as simrank_sets.h: 0 or a negative status (SIMRANK_RANK_ERR_*), the message of the last failure on the
 * calling thread from simrank_rank_last_error(); device pointers are HIP device memory of the current device; `stream` is
 * a hipStream_t passed as void*; every entry point only queues work on it and allocates nothing.  Independent of the
 * other headers of this project: this one includes none of them and the library links none of their libraries.
 */
#ifndef SIMRANK_RANK_H
#define SIMRANK_RANK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMRANK_RANK_VERSION 1
#define SIMRANK_RANK_CHUNK 1024        /* band columns of one workgroup: 256 lanes x 4 */
#define SIMRANK_RANK_TILE 256          /* targets of a basket staged through local memory together */
#define SIMRANK_RANK_MAX_BLOCKS (1 << 24)   /* workgroups of one call: 2^32 work-items are never reached */

#if defined(__GNUC__)
#define SIMRANK_RANK_API __attribute__((visibility("default")))
#else
#define SIMRANK_RANK_API
#endif

enum {
    SIMRANK_RANK_OK = 0,
    SIMRANK_RANK_ERR_INVALID = -1,     /* bad argument: NULL, shape, too many workgroups */
    SIMRANK_RANK_ERR_HIP = -2          /* a HIP runtime call failed */
};

SIMRANK_RANK_API int simrank_rank_version(void);
SIMRANK_RANK_API const char* simrank_rank_last_error(void);

/* Workgroups simrank_rank_count launches for n_sets baskets over n_out band columns; -1 for bad arguments.  A caller
 * cuts its baskets into bands so that this stays at or below SIMRANK_RANK_MAX_BLOCKS. */
SIMRANK_RANK_API int64_t simrank_rank_blocks(int64_t n_sets, int64_t n_out);

/* For every basket q < n_sets and every target x of it with 0 <= tgt_col[x] < n_out:
 *     tgt_score[x] = band[q * ld_band + tgt_col[x]]
 * Every other entry of tgt_score is left untouched: the one block that holds a target's column reports its score to all
 * blocks.  One wave per basket. */
SIMRANK_RANK_API int simrank_rank_gather(const double* band, int64_t ld_band, int64_t n_sets, int64_t n_out,
                                         const int64_t* tgt_ptr, const int32_t* tgt_col, double* tgt_score,
                                         void* stream);

/* For every basket q < n_sets that has targets, with v_c = band[q * ld_band + c] and id(c) = col_ids[c] (device int32),
 * or c when col_ids is NULL:
 *     candidates[q] += the number of columns c < n_out with v_c > -inf
 *     before[x]     += the number of columns c < n_out with v_c > -inf and
 *                      (v_c > tgt_score[x], or v_c == tgt_score[x] and id(c) < tgt_id[x])       for every target x of q
 * in IEEE double comparisons: v > -inf is false for NaN and for the -inf of an excluded column, as simrank_sets_topk
 * tests a candidate; -0.0 == +0.0 ties; the target's own column never counts, its id being no smaller than itself.  A
 * target whose score is NaN receives 0, one whose score is -inf the number of candidates: such a target is no candidate
 * itself, which its score tells the caller.  `before` and `candidates` are device int64 and are ADDED to with integer
 * atomics, so the result does not depend on the schedule.  A basket without targets reads nothing of the band and adds
 * nothing, not to candidates[q] either.
 *
 * One workgroup owns one basket and SIMRANK_RANK_CHUNK band columns; a lane keeps its 4 values and ids in registers
 * while the basket's targets pass through local memory in tiles of SIMRANK_RANK_TILE; a wave's predicates are counted
 * with one ballot each and reach memory as one 64-bit add per target and workgroup.  The cost is T_q x n_out
 * comparisons for a basket of T_q targets: meant for tens or hundreds of targets per basket, not for thousands. */
SIMRANK_RANK_API int simrank_rank_count(const double* band, int64_t ld_band, int64_t n_sets, int64_t n_out,
                                        const int32_t* col_ids, const int64_t* tgt_ptr, const double* tgt_score,
                                        const int32_t* tgt_id, int64_t* before, int64_t* candidates, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SIMRANK_RANK_H */
