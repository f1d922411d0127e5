// One SIDE of a single-GPU fit: one similarity matrix (n x n, ping-pong, panel-blocked, in the solver's node order) with
// everything its update needs — the n x k pattern, the transposed product, evidence counts, prior, node orders — and the
// functions over it.  simrank_plan (plan.hip) holds one side with k = n, which is its own operand; simrank_biplan
// (biplan.hip) holds two, each the other's operand.  Counters, events, the stream and the loop belong to the plan.
// Included by plan.hip and biplan.hip only; exports nothing.
#pragma once
#include <cstring>
#include <vector>

#include "common.h"

namespace simrank {

constexpr float kHalfScale = 16384.0f;        // what fp16-held matrices are scaled by (include/simrank_hip.h, SCALE)

// as SR_HIP, with "out of memory" told apart
#define SIDE_HIP(call)                                                                            \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            (void)hipGetLastError();                                                              \
            return e_ == hipErrorOutOfMemory ? SIMRANK_ERR_ALLOC : SIMRANK_ERR_HIP;               \
        }                                                                                         \
    } while (0)

struct side_t {
    int64_t n = 0, k = 0, rows_pad = 0, k_rows_pad = 0;    // n: own group, k: the operand's (the other group; one matrix: n)
    size_t mat_bytes = 0, t_bytes = 0;
    simrank_graph* g = nullptr;                // n x k, solver order on both sides
    float* S[2] = {nullptr, nullptr};          // n x n, panel-blocked, ping-pong
    float* Tt = nullptr;                       // k x n: (W . S_operand)^T
    uint8_t* ev = nullptr;                     // evidence counts (SimRank++), panel-blocked u8
    float* prior = nullptr;                    // panel-blocked, solver order
    int32_t* inv = nullptr;                    // device: position of caller's node i in the solver's order
    int32_t* ord_dev = nullptr;                // device: caller's node at position r (ids of the columns: top-k, "ids")
    std::vector<int32_t> ord;                  // host copy
    float coef = 0.8f, lbd = 0.f;
    int32_t restrict_support = 0;
    int32_t half = 0;                          // 1: S and Tt are fp16 on 64-column panels (half.hip), value x kHalfScale
    int cur = 0;                               // S[cur] is the current iterate
    // leg 1 in front of a triangle-form leg 2 (simrank_plan only; planprep.hip first_block_table): per panel of Tt's rows the
    // first 128-row block of leg 1 that leg 2 reads — device copy for the kernel, host copy for the counts
    int32_t* first_block = nullptr;
    std::vector<int32_t> first_block_host;
    int64_t leg1_units = 0, leg1_skipped = 0;  // of the latest update: workgroups of the one-launch leg 1 that have a unit, and
                                               // how many of them returned at once ("leg1_units", "leg1_skipped")
    int64_t leg2_short_groups = 0;             // of the latest update: short groups its leg 2 took ("leg2_short_groups")
    int64_t dead_units = -1;                   // what the table skips of such a launch (-1: not counted yet)
};

// an n x n f32 matrix on 32-column panels: the prior, and the widened copy of an fp16-held iterate
inline size_t side_f32_bytes(const side_t& a) { return size_t((a.n + 31) / 32) * size_t(a.rows_pad) * 32 * sizeof(float); }

inline void side_shape(side_t& a, int64_t n, int64_t k, bool half) {
    a.n = n;
    a.k = k;
    a.half = half ? 1 : 0;
    a.rows_pad = (n + 7) / 8 * 8 + 8;
    a.k_rows_pad = (k + 7) / 8 * 8 + 8;
    // (fp16: 64-column panels of 2-byte elements — a row segment is 128 bytes either way)
    const size_t panels = half ? size_t((n + 63) / 64) : size_t((n + 31) / 32);
    a.mat_bytes = panels * size_t(a.rows_pad) * 128;        // n x n
    a.t_bytes = panels * size_t(a.k_rows_pad) * 128;        // k x n
}

// The matrices and both node orders; the stream is drained (inv may be a host vector about to go away).
// (no memset: reset fills S[0] — zeros and the diagonal —, every update writes all of the other iterate and every tile of Tt
// that its leg 2 reads before anything reads them — a leg 1 in front of a triangle-form leg 2 leaves the tiles that leg never
// reads as they are (side_leg_pair) —, and the padding rows and columns of a panel are read by nobody: lanes that hold
// columns past the edge compute on whatever is there and never store.  Three 17 GiB memsets were 10 ms of a config-5 set-up.)
inline int side_alloc(side_t& a, const std::vector<int32_t>& ord, const std::vector<int32_t>& inv, hipStream_t st) {
    const size_t ids = size_t(a.n) * sizeof(int32_t);
    for (float** b : {&a.S[0], &a.S[1]}) SIDE_HIP(pool_hip_alloc((void**)b, a.mat_bytes));
    SIDE_HIP(pool_hip_alloc((void**)&a.Tt, a.t_bytes));
    SIDE_HIP(pool_hip_alloc((void**)&a.inv, ids));
    SIDE_HIP(hipMemcpyAsync(a.inv, inv.data(), ids, hipMemcpyHostToDevice, st));
    a.ord = ord;
    SIDE_HIP(pool_hip_alloc((void**)&a.ord_dev, ids));
    SIDE_HIP(hipMemcpyAsync(a.ord_dev, a.ord.data(), ids, hipMemcpyHostToDevice, st));
    SIDE_HIP(hipStreamSynchronize(st));
    return SIMRANK_OK;
}

// what a finished fit no longer needs: the iterates, the transposed product, the prior (the evidence counts and the
// node orders stay: *_evidence_u8 reads them later — the estimators' lazy `Evidence` attribute)
inline void side_trim(side_t& a) {
    (void)pool_free(a.S[0]); (void)pool_free(a.S[1]); (void)pool_free(a.Tt); (void)pool_free(a.prior);
    a.S[0] = a.S[1] = a.Tt = a.prior = nullptr;
}

inline void side_free(side_t& a) {
    side_trim(a);
    (void)pool_free(a.ev); (void)pool_free(a.inv); (void)pool_free(a.ord_dev); (void)pool_free(a.first_block);
    simrank_graph_destroy(a.g);
}

inline int side_reset(side_t& a, hipStream_t st) {
    a.cur = 0;
    if (a.half) return simrank_fill_identity_blocked_h16(a.S[0], a.n, a.n, a.rows_pad, 0, kHalfScale, st);
    return simrank_fill_identity_blocked(a.S[0], a.n, a.n, a.rows_pad, 0, st);
}

// the evidence counts' block, every byte `fill` (0: to be counted into — simrank_evidence_counts_blocked)
inline int side_evidence_alloc(side_t& a, int fill, hipStream_t st) {
    const size_t ev_bytes = size_t((a.n + 31) / 32) * size_t(a.rows_pad) * 32;
    hipError_t e = pool_hip_alloc((void**)&a.ev, ev_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(a.ev, fill, ev_bytes, st);
    if (e != hipSuccess) {
        set_error("evidence counts: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? SIMRANK_ERR_ALLOC : SIMRANK_ERR_HIP;
    }
    return SIMRANK_OK;
}

// the side's choice of the restricted leg 2 from the live segments of its counts
inline int side_restrict(side_t& a, hipStream_t st) {
    int64_t live = 0, total = 1;
    const int rc = simrank_evidence_live_segments(a.ev, 32, a.rows_pad, a.n, a.n, &live, &total, st);
    if (rc) return rc;
    a.restrict_support = restrict_choice(a.g->tun, live, total);
    return SIMRANK_OK;
}

// host n x n (caller's order) -> device row-major -> panel-blocked in the solver's order
inline int side_prior(side_t& a, const float* apriori, int64_t ld_apriori, hipStream_t st) {
    const int64_t n = a.n;
    float* tmp = nullptr;
    SIDE_HIP(pool_hip_alloc((void**)&tmp, size_t(n) * size_t(n) * sizeof(float)));
    hipError_t e = pool_hip_alloc((void**)&a.prior, side_f32_bytes(a));
    if (e == hipSuccess) e = hipMemsetAsync(a.prior, 0, side_f32_bytes(a), st);
    if (e == hipSuccess) e = hipMemcpy2DAsync(tmp, size_t(n) * 4, apriori, size_t(ld_apriori) * 4, size_t(n) * 4, size_t(n),
                                              hipMemcpyHostToDevice, st);
    int rc = SIMRANK_OK;
    if (e == hipSuccess) {
        // dst[i][j] = src[ord[i]][ord[j]]
        rc = simrank_permute_layout(tmp, n, 0, a.prior, 32, a.rows_pad, n, n, a.ord_dev, a.ord_dev, 4, st);
        e = hipStreamSynchronize(st);
    }
    (void)pool_free(tmp);
    if (e != hipSuccess) {
        set_error("plan prior upload: %s", hipGetErrorString(e));
        return SIMRANK_ERR_HIP;
    }
    return rc;
}

// One update of side `a` from the current iterate of its operand side `o` (a itself: one matrix), as two launches — leg 1:
// Tt (k x n) = (W . S_o)^T, fused_trans_kernel; leg 2: the upper-triangle gather with the fused epilogue and count — into
// a.S[a.cur ^ 1]; the striped counts go to `host_slot` (pinned) behind it.  a.cur stays: the caller adopts the update.
// from_identity: S_o is the identity, so leg 1 is W^T written directly — the same bits without a gather.
// asym: the iterates are not symmetric (a prior that is not): leg 2 = leg 1's launch again, then the epilogue as a pass
// of its own.  stamp() is called before leg 1, between the legs and after leg 2 (simrank_plan_set_timing).
// A side with a first_block table (simrank_plan): where the leg 2 of THIS update is a triangle form — asked of spmm.hip's
// dispatch with leg 2's own arguments, from the knobs as they are now — leg 1 leaves out the units that form never reads
// (tuning "leg1_skip").  Never for the identity's leg 1, an asymmetric prior (leg 2 runs leg 1's kernel over all of Tt),
// fp16-held matrices, or a leg 1 that is not the one-launch kernel.
template <class Stamp>
int side_leg_pair(side_t& a, const side_t& o, bool from_identity, bool asym, double eps, int32_t exact_count,
                  unsigned long long* counters, unsigned long long* host_slot, hipStream_t st, Stamp&& stamp) {
    const int nx = a.cur ^ 1;
    simrank_epilogue ep{};
    ep.coef = a.coef;
    ep.lbd = a.lbd;
    ep.evidence = a.ev;
    ep.ld_evidence = 32;
    ep.apriori = a.prior;
    ep.ld_apriori = 32;
    ep.previous = a.S[a.cur];
    ep.ld_previous = 32;
    ep.eps = eps;
    ep.n_changed = counters;
    ep.diag_col0 = 0;
    ep.set_diag = 1;
    ep.symmetric = 1;
    ep.restrict_support = a.restrict_support;
    ep.count_any = exact_count ? 0 : 1;
    const int32_t* skip = nullptr;
    if (a.first_block && a.g->tun.leg1_skip && !from_identity && !asym && !a.half) {
        bool triangle = false;
        const int rct = spmm_blocked_is_triangle(a.g, a.Tt, a.k_rows_pad, a.n, a.S[nx], a.rows_pad, &ep, &triangle);
        if (rct) return rct;
        if (triangle) skip = a.first_block;
    }
    int rc = stamp();
    if (rc) return rc;
    bool skipping = false;
    rc = from_identity ? (a.half ? identity_leg1_blocked_h16(a.g, reinterpret_cast<uint16_t*>(a.Tt), a.k_rows_pad, kHalfScale, st)
                                 : identity_leg1_blocked(a.g, a.Tt, a.k_rows_pad, st))
         : a.half ? simrank_spmm_blocked_h16(a.g, o.S[o.cur], o.rows_pad, a.k, a.Tt, a.k_rows_pad, 1, nullptr, 0, kHalfScale, st)
                  : spmm_blocked_leg1(a.g, o.S[o.cur], o.rows_pad, a.k, a.Tt, a.k_rows_pad, skip, &skipping, st);
    a.leg1_units = a.leg1_skipped = 0;
    if (!rc && a.first_block && !from_identity && !a.half) {
        int64_t dead = 0;
        fused_leg1_counts(a.g, a.k, skipping ? a.first_block_host.data() : nullptr, &a.leg1_units, &dead);
        if (skipping) {
            if (a.dead_units < 0) a.dead_units = dead;
            a.leg1_skipped = a.dead_units;
        }
    }
    if (!rc) rc = stamp();
    if (rc) return rc;
    if (asym) {
        // S is not symmetric (SimRank.py:453, :488, :491 with a prior that is not): W . Tt is the TRANSPOSE of W S_o W^T, so
        // leg 2 is leg 1's launch on Tt — X -> (W X)^T, the one-launch kernel again — and the epilogue (coefficient,
        // evidence, prior, diagonal, exact count) runs over the stored product in place
        ep.symmetric = 0;
        ep.restrict_support = 0;
        rc = simrank_spmm_blocked(a.g, a.Tt, a.k_rows_pad, a.n, a.S[nx], a.rows_pad, 1, nullptr, st);
        if (!rc) rc = simrank_epilogue_apply_blocked(a.S[nx], a.S[nx], a.n, a.n, a.rows_pad, &ep, st);
    } else {
        rc = a.half ? simrank_spmm_blocked_h16(a.g, a.Tt, a.k_rows_pad, a.n, a.S[nx], a.rows_pad, 0, &ep, a.rows_pad, kHalfScale, st)
                    : simrank_spmm_blocked(a.g, a.Tt, a.k_rows_pad, a.n, a.S[nx], a.rows_pad, 0, &ep, st);
    }
    // (the launch's answer, copied while this update is the graph's latest launch: the side owns its graph)
    a.leg2_short_groups = (asym || a.half || rc) ? 0 : a.g->leg2_short_taken;
    if (!rc) rc = stamp();
    if (rc) return rc;
    SR_HIP(hipMemcpyAsync(host_slot, counters, sizeof(unsigned long long) * SIMRANK_CHANGED_SLOTS, hipMemcpyDeviceToHost, st));
    return SIMRANK_OK;
}

// The current iterate as f32 panels: itself, or (fp16-held) a widened copy in *scratch, which the caller frees once its
// work on the stream is done.
inline int side_f32(const side_t& a, hipStream_t st, const float** src, float** scratch) {
    *src = a.S[a.cur];
    *scratch = nullptr;
    if (!a.half) return SIMRANK_OK;
    SR_HIP(pool_hip_alloc((void**)scratch, side_f32_bytes(a)));
    *src = *scratch;
    return simrank_widen_blocked_h16(a.S[a.cur], a.rows_pad, *scratch, a.rows_pad, a.n, a.n, kHalfScale, st);
}

// dst[i][j] = S[inv[i]][inv[j]]: out of the panel-blocked layout and the solver's node order band by band (handback.hip),
// FULL form (mode 0): every element crosses PCIe.  The symmetric form (upper triangle over PCIe, mirrored by the host
// threads) is opt-in (SIMRANK_SYM_HANDBACK=1) and checks its premise on the device first — a plan with an asymmetric
// prior has asymmetric iterates (SimRank.py:453), and even symmetric ones are bitwise symmetric only outside the
// diagonal tiles.
inline int side_result_f64(const side_t& a, double* dst, int64_t ld, hipStream_t st) {
    const float* src = nullptr;
    float* wide = nullptr;
    int rc = side_f32(a, st, &src, &wide);
    if (!rc) rc = simrank_handback_f64(dst, ld, src, 32, a.rows_pad, a.n, a.inv, 0, st);
    (void)hipStreamSynchronize(st);
    (void)pool_free(wide);
    return rc;
}

inline int side_rows_f32(const side_t& a, const int32_t* rows, int32_t n_rows, float* dst, int64_t ld, hipStream_t st) {
    return rows_to_host(a.S[a.cur], a.rows_pad, a.n, a.inv, rows, n_rows, dst, ld, a.half ? 2 : 4, kHalfScale, st);
}

// dst[i][j] = counts[inv[i]][inv[j]] (saturated at 255; Evidence = 1 - 0.5 ** count, SimRank.py:316)
inline int side_evidence_u8(const side_t& a, uint8_t* dst, int64_t ld, hipStream_t st, const char* who) {
    uint8_t* tmp = nullptr;
    SR_HIP(pool_hip_alloc((void**)&tmp, size_t(a.n) * size_t(a.n)));
    const int rc = simrank_permute_layout(a.ev, 32, a.rows_pad, tmp, a.n, 0, a.n, a.n, a.inv, a.inv, 1, st);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpy2DAsync(dst, size_t(ld), tmp, size_t(a.n), size_t(a.n), size_t(a.n), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)pool_free(tmp);
    if (e != hipSuccess || e2 != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(e != hipSuccess ? e : e2));
        return SIMRANK_ERR_HIP;
    }
    return rc;
}

// The selection runs on the side's own panel-blocked matrix in the solver's order (one pass, eight rows per wave;
// fp16-held: on its f32 copy), reporting the caller's ids; the rows go back into the caller's order on the host —
// 2 x n x k values across PCIe instead of n^2, and no n^2 copy on the device either.
inline int side_topk(const side_t& a, int32_t k, int32_t exclude_diag, int32_t* idx_host, float* val_host, hipStream_t st,
                     const char* who) {
    const int64_t n = a.n;
    float* wide = nullptr;
    int32_t* idx_dev = nullptr;
    float* val_dev = nullptr;
    hipError_t e = hipSuccess;
    int rc = SIMRANK_OK;
    if (a.half) {
        e = pool_hip_alloc((void**)&wide, side_f32_bytes(a));
        if (e == hipSuccess) rc = simrank_widen_blocked_h16(a.S[a.cur], a.rows_pad, wide, a.rows_pad, n, n, kHalfScale, st);
    }
    if (e == hipSuccess) e = pool_hip_alloc((void**)&idx_dev, size_t(n) * size_t(k) * sizeof(int32_t));
    if (e == hipSuccess) e = pool_hip_alloc((void**)&val_dev, size_t(n) * size_t(k) * sizeof(float));
    std::vector<int32_t> idx_s;
    std::vector<float> val_s;
    if (e == hipSuccess && !rc) {
        // (the diagonal of the solver's order is the diagonal of the caller's: position r against position r)
        rc = simrank_topk_rows_blocked(a.half ? wide : a.S[a.cur], a.rows_pad, n, n, 0, a.ord_dev, k, exclude_diag, idx_dev,
                                       val_dev, st);
        idx_s.resize(size_t(n) * size_t(k));
        val_s.resize(size_t(n) * size_t(k));
    }
    if (e == hipSuccess && !rc)
        e = hipMemcpyAsync(idx_s.data(), idx_dev, size_t(n) * size_t(k) * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !rc)
        e = hipMemcpyAsync(val_s.data(), val_dev, size_t(n) * size_t(k) * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    else (void)hipStreamSynchronize(st);
    (void)pool_free(wide); (void)pool_free(idx_dev); (void)pool_free(val_dev);
    if (e != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(e));
        (void)hipGetLastError();
        return SIMRANK_ERR_HIP;
    }
    if (rc) return rc;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t node = a.ord[(size_t)r];
        std::memcpy(idx_host + node * k, idx_s.data() + r * k, size_t(k) * sizeof(int32_t));
        std::memcpy(val_host + node * k, val_s.data() + r * k, size_t(k) * sizeof(float));
    }
    return SIMRANK_OK;
}

inline int side_get(const side_t& a, const char* key, int64_t* value) {
    if (!strcmp(key, "restrict_support")) *value = a.restrict_support;
    else if (!strcmp(key, "iterate")) *value = (int64_t)(uintptr_t)a.S[a.cur];
    else if (!strcmp(key, "iterate_layout")) *value = a.half ? 2 : 0;
    else if (!strcmp(key, "iterate_stride")) *value = a.rows_pad;
    else if (!strcmp(key, "iterate_rows") || !strcmp(key, "iterate_col_hi")) *value = a.n;
    else if (!strcmp(key, "iterate_col_lo")) *value = 0;
    else if (!strcmp(key, "ids")) *value = (int64_t)(uintptr_t)a.ord_dev;
    else if (!strcmp(key, "leg1_units")) *value = a.leg1_units;
    else if (!strcmp(key, "leg1_skipped")) *value = a.leg1_skipped;
    else if (!strcmp(key, "leg2_short_groups")) *value = a.leg2_short_groups;
    else if (!strcmp(key, "graph")) *value = (int64_t)(uintptr_t)a.g;
    else SR_REQUIRE(false, "unknown plan key '%s'", key);
    return SIMRANK_OK;
}

}  // namespace simrank
