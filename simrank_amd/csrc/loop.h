// The reference's loop, once: what simrank_plan_run_cb, simrank_biplan_run_cb, simrank_shardplan_run and
// simrank_shardbiplan_run share.  Plain host C++ (nothing of HIP, nothing of common.h): tools/host/loop_check.cpp drives
// it with a scripted fake under the sanitizers (make loop_check).
//
//     for k in range(iterations):                 SimRank.py:129-140, :288-302
//         if converged(old, new): break           loop index 0 compares the identity with zeros: "converged" unless 1 > eps
//         update_progress(k / iterations)
//         new = update(old)                       no test after the last update
//
// Update k is the k-th since reset and c_k its count of changed elements.  A plan supplies
//
//     int  queue(int slot)              queue the next update; its count goes to counter slot `slot` (0 / 1, alternating)
//     int  count(int slot, bool* zero)  wait for the count in `slot` (that update only, not what was queued behind it)
//     void adopt()                      the oldest queued update that is not yet adopted becomes the current iterate
//     int  drop()                       the speculative update (queued, never adopted) is abandoned: afterwards the
//                                       current iterate is the last adopted one again
//
// With `speculate`, update k + 1 is queued BEFORE c_k is read (common.h kSpeculateBelow: the host never leaves the device
// idle to learn whether it may go on) and dropped when c_k == 0 or the caller ends the loop; without it, update k + 1 is
// queued once progress(k, 0) has returned 0.  c_k is read after update k is queued and before update k + 2 is, so two
// slots suffice.  A nonzero code from queue / count / drop is returned at once and nothing more is called.
#pragma once
#include <cstdint>

namespace simrank {

// progress(user, k, 0): loop index k goes on to an update (SimRank.py:135 `update_progress(k / iterations)`);
// progress(user, k, 1): the test passed at loop index k (:131-133).  A nonzero return value ends the loop there.
// (simrank_progress_fn of simrank_hip.h; may be null)
using loop_progress_fn = int32_t (*)(void* user, int32_t k, int32_t converged);

struct LoopResult {
    int32_t done = 0;    // updates adopted: the current iterate is the result of update `done`
    int32_t conv = -1;   // loop index at which the test passed, -1: never
    int rc = 0;          // first nonzero code of queue / count / drop (done and conv: as far as the loop got)
};

template <class Ops>
LoopResult run_loop(Ops&& ops, int32_t iterations, double eps, bool speculate, loop_progress_fn progress, void* user) {
    LoopResult r;
    auto tell = [&](int32_t k, int32_t converged) { return progress ? progress(user, k, converged) : 0; };
    if (iterations <= 0) return r;
    if (!(1.0 > eps)) {                              // (NaN included)
        r.conv = 0;
        (void)tell(0, 1);
        return r;
    }
    if (tell(0, 0) != 0) return r;
    if ((r.rc = ops.queue(1)) != 0) return r;        // update 1
    for (int32_t k = 1;; ++k) {
        // updates 1 .. k are queued, 1 .. k - 1 adopted; the count of update k is on its way into slot k & 1
        ops.adopt();
        r.done = k;
        if (k == iterations) break;                  // the reference makes no test after its last update
        if (speculate && (r.rc = ops.queue((k + 1) & 1)) != 0) return r;
        bool zero = false;
        if ((r.rc = ops.count(k & 1, &zero)) != 0) return r;
        if (zero) {                                  // converged at loop index k: k updates applied
            r.conv = k;
            (void)tell(k, 1);
        }
        if (zero || tell(k, 0) != 0) {               // (or the caller ends the loop: k updates applied)
            if (speculate) r.rc = ops.drop();
            break;
        }
        if (!speculate && (r.rc = ops.queue((k + 1) & 1)) != 0) return r;
    }
    return r;
}

}  // namespace simrank
