// The loop of BipartiteSimRank.fit / BipartiteSimRankPP.fit / BipartitleAprioriSimRank.fit behind the C ABI
// (create_plan(N or (n1, n2)) / step / download), the two-matrix twin of plan.hip:
//
//     for k in range(iterations):                               SimRank.py:288-302 (:410-424, :478-492)
//         if converged(S1_old, S1) and converged(S2_old, S2): break
//         S1 = E1 * C1 * W12.S2.W12^T (+ lbd1 A1); diag <- 1       the group-1 update reads S2 of the iteration before,
//         S2 = E2 * C2 * W21.S1.W21^T (+ lbd2 A2); diag <- 1       the group-2 update the NEW S1 (Gauss-Seidel, :300-302)
//
// One edge set describes both patterns: W12 = diag(rowscale1) . A (n1 x n2), W21 = diag(rowscale2) . A^T.
// Each update is two launches (leg 1: fused_trans_kernel on a rectangular pattern, leg 2: upper-triangle gather
// with the fused epilogue and count); iteration k + 1 is queued before the counts of iteration k are read, as in
// plan.hip (the loop itself is loop.h's; a matrix and the functions over it are side.h's, group w's operand being the
// other group's side).  Evidence: by default the corrected form — E1 from the group-1 pattern, E2 from the group-2 pattern.
// options.strict_reference = 1 is the reference's own behaviour (SimRank.py:420-423, :488-491, SURVEY.md quirk
// Q2): BOTH updates are multiplied by Evidence_N1, position by position in the caller's node order — n1 = n2:
// the group-2 update is gated by the counts of the group-1 pattern; n1 = 1: NumPy broadcasts the 1 x 1 array,
// one count gates every element; otherwise NumPy raises "operands could not be broadcast together" when the
// first group-2 update RUNS (iterations = 0 or eps >= 1 still return the identities): so do step / run here.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include <chrono>
#include <string>
#include <thread>

#include "loop.h"
#include "side.h"

using simrank::side_t;

struct simrank_biplan {
    side_t s[2];
    unsigned long long* counters = nullptr;                          // device, SIMRANK_CHANGED_SLOTS (zeroed per leg 2)
    unsigned long long* host_counters[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [iteration & 1][side]
    hipEvent_t counted[2] = {nullptr, nullptr};                      // both counts of an iteration have landed
    hipStream_t stream = nullptr;
    int32_t updates = 0;
    int32_t broadcast_error = 0;     // strict_reference with evidence and n1 != n2, n1 != 1 (quirk Q2)
    int32_t asym = 0;                // a prior of either group is not symmetric: both iterates are asymmetric (un-fused epilogue)
    int32_t identity_leg1 = 1;       // group 1's first update reads S2 = I: its leg 1 is W12^T written directly (SIMRANK_IDENTITY_LEG1=0: off)
    int32_t at_identity = 0;         // S2 is the identity (reset), no update queued since
};

namespace simrank {

static int side_update(simrank_biplan* p, int w, double eps, int32_t exact_count, unsigned long long* host_slot) {
    side_t& a = p->s[w];
    // S_other is the identity for the very first update of group 1 (SimRank.py:280-285: group 2's first update already reads
    // the new S1)
    const bool from_identity = w == 0 && p->at_identity && p->identity_leg1;
    if (w == 0) p->at_identity = 0;
    const int rc = side_leg_pair(a, p->s[w ^ 1], from_identity, p->asym != 0, eps, exact_count, p->counters, host_slot, p->stream,
                                 [] { return SIMRANK_OK; });
    if (rc) return rc;
    a.cur ^= 1;              // (the group-2 update of the same iteration reads the new S1)
    return SIMRANK_OK;
}

// one loop body: both updates, counts into slot `it`
static int iteration(simrank_biplan* p, double eps, int32_t exact_count, int it) {
    // (the reference has updated S1 when NumPy raises at :423 / :491; nobody sees that S1: the exception ends fit)
    SR_REQUIRE(!p->broadcast_error, "operands could not be broadcast together with shapes (%lld,%lld) (%lld,%lld) ",
               (long long)p->s[0].n, (long long)p->s[0].n, (long long)p->s[1].n, (long long)p->s[1].n);
    int rc = side_update(p, 0, eps, exact_count, p->host_counters[it][0]);
    if (!rc) rc = side_update(p, 1, eps, exact_count, p->host_counters[it][1]);
    if (rc) return rc;
    SR_HIP(hipEventRecord(p->counted[it], p->stream));
    return SIMRANK_OK;
}

static int read_counts(simrank_biplan* p, int it, unsigned long long* c1, unsigned long long* c2) {
    SR_HIP(hipEventSynchronize(p->counted[it]));
    unsigned long long t[2] = {0, 0};
    for (int w = 0; w < 2; ++w)
        for (int i = 0; i < SIMRANK_CHANGED_SLOTS; ++i) t[w] += p->host_counters[it][w][i];
    *c1 = t[0];
    *c2 = t[1];
    return SIMRANK_OK;
}

}  // namespace simrank

using namespace simrank;

extern "C" {

int simrank_biplan_destroy(simrank_biplan* p) {
    if (!p) return SIMRANK_OK;
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (side_t& a : p->s) side_free(a);
    (void)pool_free(p->counters);
    for (int i = 0; i < 2; ++i) {
        for (int w = 0; w < 2; ++w)
            if (p->host_counters[i][w]) (void)hipHostFree(p->host_counters[i][w]);
        if (p->counted[i]) (void)hipEventDestroy(p->counted[i]);
    }
    delete p;
    return SIMRANK_OK;
}

int simrank_biplan_reset(simrank_biplan* p) {
    SR_REQUIRE(p, "plan is NULL");
    SR_REQUIRE(p->s[0].S[0], "the plan's matrices were released (simrank_biplan_trim)");
    p->updates = 0;
    p->at_identity = 1;
    for (side_t& a : p->s) {
        const int rc = side_reset(a, p->stream);
        if (rc) return rc;
    }
    return SIMRANK_OK;
}

int simrank_biplan_create(int64_t n1, int64_t n2, int64_t nnz, const int32_t* rowptr12, const int32_t* col12,
                          const float* rowscale1, const float* rowscale2, const simrank_biplan_options* opt,
                          void* stream, simrank_biplan** out) {
    SR_REQUIRE(out, "out is NULL");
    *out = nullptr;
    const bool timed = std::getenv("SIMRANK_TIME_BUILD") != nullptr;     // diagnostic: phase durations on stderr
    const auto t_start = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (timed)
            std::fprintf(stderr, "simrank_biplan_create: %6.1f ms  %s\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(), what);
    };
    BiPlanPrep pp;
    {
        const int rc = biplan_prepare(n1, n2, nnz, rowptr12, col12, rowscale1, rowscale2, opt, &pp);   // (planprep.hip)
        if (rc) return rc;
    }
    lap("validated, ordered, both patterns renamed");
    const float* priors[2] = {opt->apriori1, opt->apriori2};
    const int64_t lds[2] = {opt->ld_apriori1, opt->ld_apriori2};
    const int64_t ns[2] = {n1, n2};
    const std::vector<int32_t>* ord = pp.ord;
    const std::vector<int32_t>* inv = pp.inv;
    simrank_biplan* p = new simrank_biplan;
    p->stream = as_stream(stream);
    p->asym = pp.asym ? 1 : 0;
    if (const char* e = std::getenv("SIMRANK_IDENTITY_LEG1")) p->identity_leg1 = (*e == '0') ? 0 : 1;
    auto fail = [&](int code) { simrank_biplan_destroy(p); return code; };
    {
        // The two graph objects are independent of each other: on graphs large enough for threads to pay the second one is
        // created on a thread beside the first (MovieLens-shaped: 9.4 + 7.9 ms one after the other).  As in plan.hip: leg 1 of
        // both groups is the one-launch kernel wherever spmm.hip's conditions hold, so the dense-block plan could only serve
        // the upper-triangle leg 2 — built only if that leg would take it (dense_lazy).
        Tuning tw[2] = {tuning_snapshot(), Tuning()};
        tw[1] = tw[0];
        int rcs[2] = {SIMRANK_OK, SIMRANK_OK};
        std::string errs[2];
        for (int w = 0; w < 2; ++w) {
            side_t& a = p->s[w];
            side_shape(a, ns[w], ns[w ^ 1], false);
            a.coef = w == 0 ? opt->c1 : opt->c2;
            a.lbd = w == 0 ? opt->lbd1 : opt->lbd2;
            if (tw[w].fuse == 1 && ((tw[w].triangle && a.n >= 64) || p->asym) && a.k <= tw[w].fuse_max_rows &&
                (a.k_rows_pad + 1) * 128 < (int64_t(1) << 31))
                tw[w].dense_lazy = 1;
        }
        auto make = [&](int w) {
            side_t& a = p->s[w];
            rcs[w] = graph_create_with(tw[w], a.n, a.k, nnz, pp.rp[w].data(), pp.cl[w].data(), pp.rs[w].data(), &a.g);
            if (rcs[w]) errs[w] = simrank_last_error();
        };
        if (nnz >= 20000) {
            int dev = 0;
            (void)hipGetDevice(&dev);
            std::thread second([&]() {
                (void)hipSetDevice(dev);
                make(1);
            });
            make(0);
            second.join();
        } else {
            make(0);
            if (!rcs[0]) make(1);
        }
        for (int w = 0; w < 2; ++w)
            if (rcs[w]) {
                set_error("%s", errs[w].c_str());
                return fail(rcs[w]);
            }
    }
    lap("graph objects");
    auto counters = [&]() -> int {
        SIDE_HIP(pool_hip_alloc((void**)&p->counters, sizeof(unsigned long long) * SIMRANK_CHANGED_SLOTS));
        for (int i = 0; i < 2; ++i) {
            for (int w = 0; w < 2; ++w)
                SIDE_HIP(hipHostMalloc((void**)&p->host_counters[i][w], sizeof(unsigned long long) * SIMRANK_CHANGED_SLOTS,
                                       hipHostMallocPortable));
            SIDE_HIP(hipEventCreateWithFlags(&p->counted[i], hipEventDisableTiming));
        }
        return SIMRANK_OK;
    };
    int rc = counters();
    if (rc) return fail(rc);
    for (int w = 0; w < 2; ++w) {
        side_t& a = p->s[w];
        rc = side_alloc(a, ord[w], inv[w], p->stream);
        if (rc) return fail(rc);
        const bool q2 = opt->evidence && opt->strict_reference && w == 1;      // Evidence_N1 on the group-2 update
        if (q2 && n1 != n2 && n1 != 1) {
            p->broadcast_error = 1;
        } else if (opt->evidence) {
            // common-neighbour counts inside the group (SimRank.py:311-320 on this group's pattern)
            if (q2 && n1 == 1 && n2 != 1) {
                // the 1 x 1 Evidence_N1 broadcasts: the one group-1 node's count (with itself) gates every element
                const int cnt = rowscale1[0] != 0.f ? (int)std::min<int64_t>(255, nnz) : 0;
                rc = side_evidence_alloc(a, cnt, p->stream);
            } else if (q2) {
                // n1 = n2: element (i, j) of the group-2 update is multiplied by Evidence_N1[i][j], positions in the
                // caller's order: the counts of the group-1 pattern with its rows taken in THIS group's solver order
                std::vector<int32_t> rp((size_t)n1 + 1, 0), cl((size_t)std::max<int64_t>(1, nnz));
                std::vector<float> rs((size_t)n1);
                for (int64_t r = 0; r < n1; ++r) {
                    const int32_t src = ord[1][(size_t)r];
                    const int32_t b = rowptr12[src], e = rowptr12[src + 1];
                    std::copy(col12 + b, col12 + e, cl.data() + rp[(size_t)r]);
                    std::sort(cl.data() + rp[(size_t)r], cl.data() + rp[(size_t)r] + (e - b));
                    rp[(size_t)r + 1] = rp[(size_t)r] + (e - b);
                    rs[(size_t)r] = rowscale1[src];
                }
                simrank_graph* g1 = nullptr;
                rc = simrank_graph_create(n1, n2, nnz, rp.data(), cl.data(), rs.data(), &g1);
                if (rc) return fail(rc);
                rc = side_evidence_alloc(a, 0, p->stream);
                if (!rc) rc = simrank_evidence_counts_blocked(g1, 0, a.n, a.ev, a.rows_pad, p->stream);
                (void)hipStreamSynchronize(p->stream);
                simrank_graph_destroy(g1);
            } else {
                rc = side_evidence_alloc(a, 0, p->stream);
                if (!rc) rc = simrank_evidence_counts_blocked(a.g, 0, a.n, a.ev, a.rows_pad, p->stream);
            }
            if (!rc) rc = side_restrict(a, p->stream);
            if (rc) return fail(rc);
        }
        if (priors[w]) {
            rc = side_prior(a, priors[w], lds[w], p->stream);
            if (rc) return fail(rc);
        }
    }
    lap("matrices, evidence counts, live segments, priors");
    rc = simrank_biplan_reset(p);
    if (rc) return fail(rc);
    lap("reset queued");
    *out = p;
    return SIMRANK_OK;
}

int simrank_biplan_step(simrank_biplan* p, double eps, int32_t exact_count, int64_t* changed1, int64_t* changed2) {
    SR_REQUIRE(p, "plan is NULL");
    SR_REQUIRE(p->s[0].S[0], "the plan's matrices were released (simrank_biplan_trim)");
    const int rc = iteration(p, eps, exact_count, 0);
    if (rc) return rc;
    ++p->updates;
    if (changed1 || changed2) {
        unsigned long long c1 = 0, c2 = 0;
        const int rc2 = read_counts(p, 0, &c1, &c2);
        if (rc2) return rc2;
        if (changed1) *changed1 = (int64_t)c1;
        if (changed2) *changed2 = (int64_t)c2;
    }
    return SIMRANK_OK;
}

int simrank_biplan_run_cb(simrank_biplan* p, int32_t iterations, double eps, simrank_progress_fn progress, void* user,
                          int32_t* updates_done, int32_t* converged_at) {
    SR_REQUIRE(p, "plan is NULL");
    SR_REQUIRE(iterations >= 0, "iterations < 0");
    SR_REQUIRE(p->s[0].S[0], "the plan's matrices were released (simrank_biplan_trim)");
    const int rc = simrank_biplan_reset(p);
    if (rc) return rc;
    struct {
        simrank_biplan* p;
        double eps;
        int queue(int slot) { return iteration(p, eps, 0, slot); }         // (each update moves its side on to the new iterate)
        int count(int slot, bool* zero) {
            unsigned long long c1 = 0, c2 = 0;
            const int rcc = read_counts(p, slot, &c1, &c2);
            *zero = c1 == 0 && c2 == 0;                                    // SimRank.py:289: both groups
            return rcc;
        }
        void adopt() {}
        int drop() {
            // back to the iterates the speculative iteration read: it wrote the buffers of the iterates before last, the
            // current ones are untouched (the caller's closing synchronisation keeps it from outliving its inputs).
            // Flipping back is right because a queue call that returned 0 flipped each side exactly once (side_update),
            // and the loop drops only after such a call; an iteration that could end half-way would have to save `cur`.
            p->s[0].cur ^= 1;
            p->s[1].cur ^= 1;
            return SIMRANK_OK;
        }
    } ops{p, eps};
    // (iteration k + 1 before the counts of iteration k on small graphs only, common.h kSpeculateBelow)
    const LoopResult r = run_loop(ops, iterations, eps, std::max(p->s[0].n, p->s[1].n) < kSpeculateBelow, progress, user);
    if (r.rc) return r.rc;
    SR_HIP(hipStreamSynchronize(p->stream));
    p->updates = r.done;
    if (updates_done) *updates_done = r.done;
    if (converged_at) *converged_at = r.conv;
    return SIMRANK_OK;
}

int simrank_biplan_run(simrank_biplan* p, int32_t iterations, double eps, int32_t* updates_done, int32_t* converged_at) {
    return simrank_biplan_run_cb(p, iterations, eps, nullptr, nullptr, updates_done, converged_at);
}

int simrank_biplan_result_f64(simrank_biplan* p, int32_t group, double* dst, int64_t ld) {
    SR_REQUIRE(p && dst && (group == 1 || group == 2), "bad result arguments");
    side_t& a = p->s[group - 1];
    SR_REQUIRE(ld >= a.n, "ld %lld < n", (long long)ld);
    SR_REQUIRE(a.S[0], "the plan's matrices were released (simrank_biplan_trim)");
    return side_result_f64(a, dst, ld, p->stream);
}

int simrank_biplan_rows_f32(simrank_biplan* p, int32_t group, const int32_t* rows, int32_t n_rows, float* dst, int64_t ld) {
    SR_REQUIRE(p && rows && dst && (group == 1 || group == 2) && n_rows > 0, "bad row arguments");
    side_t& a = p->s[group - 1];
    SR_REQUIRE(ld >= a.n, "ld %lld < n", (long long)ld);
    SR_REQUIRE(a.S[0], "the plan's matrices were released (simrank_biplan_trim)");
    return side_rows_f32(a, rows, n_rows, dst, ld, p->stream);
}

int simrank_biplan_topk(simrank_biplan* p, int32_t group, int32_t k, int32_t exclude_diag, int32_t* idx_host, float* val_host) {
    SR_REQUIRE(p && idx_host && val_host && (group == 1 || group == 2) && k > 0 && k <= 1024, "bad top-k arguments");
    side_t& a = p->s[group - 1];
    SR_REQUIRE(a.S[0], "the plan's matrices were released (simrank_biplan_trim)");
    return side_topk(a, k, exclude_diag, idx_host, val_host, p->stream, "simrank_biplan_topk");
}

int simrank_biplan_evidence_u8(simrank_biplan* p, int32_t group, uint8_t* dst, int64_t ld) {
    SR_REQUIRE(p && dst && (group == 1 || group == 2), "bad evidence arguments");
    side_t& a = p->s[group - 1];
    SR_REQUIRE(ld >= a.n, "ld %lld < n", (long long)ld);
    SR_REQUIRE(a.ev, "no evidence counts for group %d (created without evidence, or strict_reference with n1 != n2)", group);
    // the counts that GATE this group's update (strict_reference: Evidence_N1's, position by position, for group 2 as well)
    return side_evidence_u8(a, dst, ld, p->stream, "simrank_biplan_evidence_u8");
}

int simrank_biplan_get(const simrank_biplan* p, int32_t group, const char* key, int64_t* value) {
    SR_REQUIRE(p && key && value, "NULL argument");
    SR_REQUIRE(group == 1 || group == 2, "group must be 1 or 2");
    return side_get(p->s[group - 1], key, value);
}

int simrank_biplan_trim(simrank_biplan* p) {
    SR_REQUIRE(p, "plan is NULL");
    if (p->stream) SR_HIP(hipStreamSynchronize(p->stream));
    for (side_t& a : p->s) side_trim(a);
    return SIMRANK_OK;
}

}  // extern "C"
