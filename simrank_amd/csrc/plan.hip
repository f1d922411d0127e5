// The loop of SimRank.fit behind the C ABI (create_plan / step / download): a PLAN owns
// everything one single-GPU fit needs — the graph in the solver's node order, the three panel-blocked
// matrices of an update, evidence counts, prior, the striped convergence counters — and runs
//
//     for k in range(iterations):                 SimRank.py:129-140 (:351-362, :443-454 with evidence / prior)
//         if converged(old, new): break
//         new = E * C * W.S.W^T (+ lbd A); diag <- 1
//
// as two launches per update (leg 1: fused_trans_kernel, without the units of the transposed product that leg 2 never
// reads; leg 2: upper-triangle gather with the fused epilogue and count), with update k + 1 queued BEFORE the count of update k is read (graphs below 16384 nodes,
// where an update is short; common.h kSpeculateBelow): the host never
// leaves the device idle to learn whether it may go on, and when the count says "converged" the
// speculative update is simply not adopted (it wrote the buffer of the iterate before last).
// tests/pydriver.py spells the same choreography out in Python for every world size (the suite's second opinion);
// this is the single-rank case for callers that bind the library directly (INTEGRATION.md §B,
// examples/reference_hip_stub.py).  The loop itself is loop.h's, the matrix and the functions over it side.h's.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "loop.h"
#include "side.h"

struct simrank_plan {
    simrank::side_t s;                        // the one matrix: its own operand (k = n)
    unsigned long long* counters = nullptr;   // device, SIMRANK_CHANGED_SLOTS
    unsigned long long* host_counters[2] = {nullptr, nullptr};   // pinned; update u lands in slot u & 1
    hipEvent_t counted[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    int32_t asym = 0;                         // 1: the prior is not symmetric, so the iterates are not: leg 2 = leg 1's launch again
                                              //    (its product stored transposed), then the epilogue as a pass of its own
    int32_t updates = 0;                      // updates applied since the last reset
    int32_t identity_leg1 = 1;                // the first update's leg 1 without gathers (S_0 = I; SIMRANK_IDENTITY_LEG1=0: off)
    int32_t at_identity = 0;                  // S[cur] is the identity (simrank_plan_reset), no update queued since
    // simrank_plan_set_timing: three events per update (before leg 1, between the legs, after leg 2) on the plan's stream
    std::vector<hipEvent_t> ev_pool;          // created ahead of the timed region
    std::vector<hipEvent_t> ev_used;          // 3 per timed update, in order
    bool timing = false;
};

namespace simrank {

static int stamp(simrank_plan* p) {
    if (!p->timing || p->ev_pool.empty()) return SIMRANK_OK;
    hipEvent_t e = p->ev_pool.back();
    p->ev_pool.pop_back();
    p->ev_used.push_back(e);
    SR_HIP(hipEventRecord(e, p->stream));
    return SIMRANK_OK;
}

// one update: reads S[cur], writes S[cur ^ 1]; its count lands in pinned slot `slot`
static int leg_pair(simrank_plan* p, double eps, int32_t exact_count, int slot) {
    const bool timed = p->timing && p->ev_pool.size() >= 3;
    // (the first update of a fit multiplies by the identity)
    const bool from_identity = p->at_identity && p->identity_leg1;
    p->at_identity = 0;
    const int rc = side_leg_pair(p->s, p->s, from_identity, p->asym != 0, eps, exact_count, p->counters, p->host_counters[slot],
                                 p->stream, [&] { return timed ? stamp(p) : SIMRANK_OK; });
    if (rc) return rc;
    SR_HIP(hipEventRecord(p->counted[slot], p->stream));
    return SIMRANK_OK;
}

// the count of the update that used `slot`: waits for that update only, not for what was queued behind it
static int read_count(simrank_plan* p, int slot, unsigned long long* sum) {
    SR_HIP(hipEventSynchronize(p->counted[slot]));
    unsigned long long t = 0;
    for (int i = 0; i < SIMRANK_CHANGED_SLOTS; ++i) t += p->host_counters[slot][i];
    *sum = t;
    return SIMRANK_OK;
}

}  // namespace simrank

using namespace simrank;

extern "C" {

int simrank_plan_destroy(simrank_plan* p) {
    if (!p) return SIMRANK_OK;
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    (void)pool_free(p->counters);
    for (int i = 0; i < 2; ++i) {
        if (p->host_counters[i]) (void)hipHostFree(p->host_counters[i]);
        if (p->counted[i]) (void)hipEventDestroy(p->counted[i]);
    }
    for (hipEvent_t e : p->ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->ev_used) (void)hipEventDestroy(e);
    side_free(p->s);
    delete p;
    return SIMRANK_OK;
}

int simrank_plan_create(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col, const float* rowscale,
                        const simrank_plan_options* opt, void* stream, simrank_plan** out) {
    SR_REQUIRE(out, "out is NULL");
    *out = nullptr;
    const bool timed = std::getenv("SIMRANK_TIME_BUILD") != nullptr;     // diagnostic: phase durations on stderr
    const auto t_start = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (timed)
            std::fprintf(stderr, "simrank_plan_create: %6.1f ms  %s\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(), what);
    };
    PlanPrep pp;
    int rc = plan_prepare(n, nnz, rowptr, col, rowscale, opt, &pp);     // validation, node order, renamed pattern (planprep.hip)
    if (rc) return rc;
    lap("validated, ordered, renamed");
    simrank_plan* p = new simrank_plan;
    side_t& a = p->s;
    side_shape(a, n, n, opt->storage_fp16 != 0);
    p->stream = as_stream(stream);
    a.coef = opt->coef;
    a.lbd = opt->lbd;
    p->asym = pp.asym ? 1 : 0;
    if (const char* e = std::getenv("SIMRANK_IDENTITY_LEG1")) p->identity_leg1 = (*e == '0') ? 0 : 1;
    auto fail = [&](int code) { simrank_plan_destroy(p); return code; };
    {
        Tuning t = tuning_snapshot();
        if (p->s.half) {
            t.fuse_unit = int64_t(1) << 20;      // (half.hip runs whole blocks: no units whose sums meet in memory)
            // one fp16 MFMA term instead of three bf16 ones, but an operand segment serves 64 columns, so the gathers got
            // cheaper still: the break-even moves up by one (4 is 3 % faster than 3, 2 is 12 % slower), and groups of four
            // blocks without a set beat three (7 % at config 5) — while the knobs are at their defaults (as driver.Side did)
            // (round 6, fuse_min = 0 — quads that pay: the same step up, 256 entries per quad instead of 192)
            if (t.fuse_min == 3) {
                t.fuse_min = 4;
                if (t.fuse_group == 3) t.fuse_group = 4;
            } else if (t.fuse_min == 0 && t.fuse_pays < 0) {
                t.fuse_pays = 256;
                if (t.fuse_group == 3) t.fuse_group = 4;
            }
        }
        // leg 1 = the one-launch kernel (fp16-held: always; f32: whenever spmm.hip's conditions hold), so the dense-block plan
        // could only serve the upper-triangle leg 2: built only if that leg would take it
        // (and only where that leg IS the upper-triangle one — knob on, 64 nodes or more — or stores transposed: asymmetric priors)
        if (t.fuse == 1 && ((t.triangle && n >= 64) || p->asym) &&
            (p->s.half || ((opt->dense_terms == 0 || opt->dense_terms == 3) && n <= t.fuse_max_rows &&
                         (p->s.rows_pad + 1) * 128 < (int64_t(1) << 31))))
            t.dense_lazy = 1;
        // The evidence counts (SimRank.py:311-320: common in-neighbours of the pattern; 1 - 2^-count in the epilogue) read the
        // CSR / CSC arrays only: they are queued as soon as those are on the device and run while the host threads still
        // build the tile, dense-block and one-launch plans (14 ms beside 30 at config 5).
        std::function<int(simrank_graph*)> counts = [&](simrank_graph* g) -> int {
            if (!opt->evidence) return SIMRANK_OK;
            const int rce = side_evidence_alloc(a, 0, p->stream);
            return rce ? rce : simrank_evidence_counts_blocked(g, 0, n, a.ev, a.rows_pad, p->stream);
        };
        rc = graph_create_with(t, n, n, nnz, pp.rp.data(), pp.cl.data(), pp.rs.data(), &a.g, &counts);
    }
    if (rc) return fail(rc);
    lap("graph object (evidence counts queued)");
    if (opt->dense_terms == 1) {                 // one fp16 operand term on the matrix cores (config 5's literal reading)
        rc = simrank_graph_set_dense_terms(p->s.g, 1);
        if (rc) return fail(rc);
    }
    if (p->s.half && !p->s.g->fused) {
        set_error("storage_fp16 needs the one-launch plan (tuning fuse = 1) and a graph that has one");
        return fail(SIMRANK_ERR_INVALID);
    }
    auto counters = [&]() -> int {
        SIDE_HIP(pool_hip_alloc((void**)&p->counters, sizeof(unsigned long long) * SIMRANK_CHANGED_SLOTS));
        for (int i = 0; i < 2; ++i) {
            SIDE_HIP(hipHostMalloc((void**)&p->host_counters[i], sizeof(unsigned long long) * SIMRANK_CHANGED_SLOTS, hipHostMallocPortable));
            SIDE_HIP(hipEventCreateWithFlags(&p->counted[i], hipEventDisableTiming));
        }
        return SIMRANK_OK;
    };
    rc = counters();
    if (!rc) rc = side_alloc(a, pp.ord, pp.inv, p->stream);
    if (!rc && !a.half) {
        // the units of leg 1 that a triangle-form leg 2 never reads (planprep.hip first_block_table; side_leg_pair decides per
        // update whether they are left out): one int32 per panel, the plan's, freed with the side
        auto table = [&]() -> int {
            const size_t bytes = pp.first_block.size() * sizeof(int32_t);
            SIDE_HIP(pool_hip_alloc((void**)&a.first_block, bytes));
            SIDE_HIP(hipMemcpyAsync(a.first_block, pp.first_block.data(), bytes, hipMemcpyHostToDevice, p->stream));
            SIDE_HIP(hipStreamSynchronize(p->stream));
            a.first_block_host = pp.first_block;
            return SIMRANK_OK;
        };
        rc = table();
    }
    if (rc) return fail(rc);
    lap("matrices allocated, orders uploaded, stream drained");
    if (opt->evidence) rc = side_restrict(a, p->stream);
    if (!rc && opt->apriori) rc = side_prior(a, opt->apriori, opt->ld_apriori, p->stream);
    if (rc) return fail(rc);
    lap("live segments, prior");
    rc = simrank_plan_reset(p);
    if (rc) return fail(rc);
    lap("reset queued");
    *out = p;
    return SIMRANK_OK;
}

int simrank_plan_reset(simrank_plan* p) {
    SR_REQUIRE(p, "plan is NULL");
    SR_REQUIRE(p->s.S[0], "the plan's matrices were released (simrank_plan_trim)");
    p->updates = 0;
    p->at_identity = 1;
    return side_reset(p->s, p->stream);
}

int simrank_plan_step(simrank_plan* p, double eps, int32_t exact_count, int64_t* n_changed) {
    SR_REQUIRE(p, "plan is NULL");
    SR_REQUIRE(p->s.S[0], "the plan's matrices were released (simrank_plan_trim)");
    const int rc = leg_pair(p, eps, exact_count, 0);
    if (rc) return rc;
    p->s.cur ^= 1;
    ++p->updates;
    if (n_changed) {
        unsigned long long c = 0;
        const int rc2 = read_count(p, 0, &c);
        if (rc2) return rc2;
        *n_changed = (int64_t)c;
    }
    return SIMRANK_OK;
}

int simrank_plan_run_cb(simrank_plan* p, int32_t iterations, double eps, simrank_progress_fn progress, void* user,
                        int32_t* updates_done, int32_t* converged_at) {
    SR_REQUIRE(p, "plan is NULL");
    SR_REQUIRE(iterations >= 0, "iterations < 0");
    SR_REQUIRE(p->s.S[0], "the plan's matrices were released (simrank_plan_trim)");
    const int rc = simrank_plan_reset(p);
    if (rc) return rc;
    struct {
        simrank_plan* p;
        double eps;
        int queue(int slot) { return leg_pair(p, eps, 0, slot); }          // reads S[cur], writes S[cur ^ 1]
        int count(int slot, bool* zero) {                                  // waits for that update only
            unsigned long long c = 0;
            const int rcc = read_count(p, slot, &c);
            *zero = c == 0;
            return rcc;
        }
        void adopt() { p->s.cur ^= 1; }
        int drop() { return SIMRANK_OK; }       // (it wrote the buffer of the iterate before last: S[cur] is untouched)
    } ops{p, eps};
    // (update k + 1 before the count of update k on small graphs only, common.h kSpeculateBelow)
    const LoopResult r = run_loop(ops, iterations, eps, p->s.n < kSpeculateBelow, progress, user);
    if (r.rc) return r.rc;
    SR_HIP(hipStreamSynchronize(p->stream));
    p->updates = r.done;
    if (updates_done) *updates_done = r.done;
    if (converged_at) *converged_at = r.conv;
    return SIMRANK_OK;
}

int simrank_plan_run(simrank_plan* p, int32_t iterations, double eps, int32_t* updates_done, int32_t* converged_at) {
    return simrank_plan_run_cb(p, iterations, eps, nullptr, nullptr, updates_done, converged_at);
}

int simrank_plan_result(simrank_plan* p, float* dst, int64_t ld) {
    SR_REQUIRE(p && dst && ld >= p->s.n, "bad result arguments");
    SR_REQUIRE(p->s.S[0], "the plan's matrices were released (simrank_plan_trim)");
    // dst[i][j] = S[inv[i]][inv[j]]: out of the panel-blocked layout and the solver's node order in one pass
    // (fp16-held: through an f32 panel-blocked scratch copy)
    const side_t& a = p->s;
    const float* src = nullptr;
    float* wide = nullptr;
    int rc = side_f32(a, p->stream, &src, &wide);
    if (!rc) rc = simrank_permute_layout(src, 32, a.rows_pad, dst, ld, 0, a.n, a.n, a.inv, a.inv, 4, p->stream);
    if (wide) {
        (void)hipStreamSynchronize(p->stream);
        (void)pool_free(wide);
    }
    return rc;
}

int simrank_plan_result_f64(simrank_plan* p, double* dst, int64_t ld) {
    SR_REQUIRE(p && dst && ld >= p->s.n, "bad result arguments");
    SR_REQUIRE(p->s.S[0], "the plan's matrices were released (simrank_plan_trim)");
    return side_result_f64(p->s, dst, ld, p->stream);
}

int simrank_plan_evidence_u8(simrank_plan* p, uint8_t* dst, int64_t ld) {
    SR_REQUIRE(p && dst && ld >= p->s.n, "bad evidence arguments");
    SR_REQUIRE(p->s.ev, "the plan was created without evidence");
    return side_evidence_u8(p->s, dst, ld, p->stream, "simrank_plan_evidence_u8");
}

int simrank_plan_trim(simrank_plan* p) {
    SR_REQUIRE(p, "plan is NULL");
    if (p->stream) SR_HIP(hipStreamSynchronize(p->stream));
    side_trim(p->s);
    return SIMRANK_OK;
}

int simrank_plan_rows_f32(simrank_plan* p, const int32_t* rows, int32_t n_rows, float* dst, int64_t ld) {
    SR_REQUIRE(p && rows && dst && n_rows > 0 && ld >= p->s.n, "bad row arguments");
    SR_REQUIRE(p->s.S[0], "the plan's matrices were released (simrank_plan_trim)");
    return side_rows_f32(p->s, rows, n_rows, dst, ld, p->stream);
}

int simrank_plan_topk(simrank_plan* p, int32_t k, int32_t exclude_diag, int32_t* idx_host, float* val_host) {
    SR_REQUIRE(p && idx_host && val_host && k > 0 && k <= 1024, "bad top-k arguments");
    SR_REQUIRE(p->s.S[0], "the plan's matrices were released (simrank_plan_trim)");
    return side_topk(p->s, k, exclude_diag, idx_host, val_host, p->stream, "simrank_plan_topk");
}

int simrank_plan_set_timing(simrank_plan* p, int32_t updates) {
    SR_REQUIRE(p && updates >= 0 && updates <= (1 << 20), "bad timing arguments");
    // events for `updates` updates are created NOW (outside whatever the caller times); 0 switches the stamps off
    for (hipEvent_t e : p->ev_used) p->ev_pool.push_back(e);
    p->ev_used.clear();
    while ((int64_t)p->ev_pool.size() < 3 * (int64_t)updates) {
        hipEvent_t e;
        SR_HIP(hipEventCreate(&e));
        p->ev_pool.push_back(e);
    }
    p->timing = updates > 0;
    return SIMRANK_OK;
}

int simrank_plan_leg_times(simrank_plan* p, double* leg1_ms, double* leg2_ms, int32_t* updates) {
    SR_REQUIRE(p, "plan is NULL");
    SR_HIP(hipStreamSynchronize(p->stream));
    double a = 0, b = 0;
    const size_t n = p->ev_used.size() / 3;
    for (size_t u = 0; u < n; ++u) {
        float t1 = 0, t2 = 0;
        SR_HIP(hipEventElapsedTime(&t1, p->ev_used[3 * u], p->ev_used[3 * u + 1]));
        SR_HIP(hipEventElapsedTime(&t2, p->ev_used[3 * u + 1], p->ev_used[3 * u + 2]));
        a += t1;
        b += t2;
    }
    if (leg1_ms) *leg1_ms = n ? a / (double)n : 0.0;
    if (leg2_ms) *leg2_ms = n ? b / (double)n : 0.0;
    if (updates) *updates = (int32_t)n;
    for (hipEvent_t e : p->ev_used) p->ev_pool.push_back(e);
    p->ev_used.clear();
    return SIMRANK_OK;
}

int simrank_plan_info(const simrank_plan* p, int64_t* n, int32_t* updates, const simrank_graph** graph) {
    SR_REQUIRE(p, "plan is NULL");
    if (n) *n = p->s.n;
    if (updates) *updates = p->updates;
    if (graph) *graph = p->s.g;
    return SIMRANK_OK;
}

int simrank_plan_get(const simrank_plan* p, const char* key, int64_t* value) {
    SR_REQUIRE(p && key && value, "NULL argument");
    return side_get(p->s, key, value);
}

}  // extern "C"
