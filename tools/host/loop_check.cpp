// Drives csrc/loop.h (the loop behind simrank_plan_run_cb, simrank_biplan_run_cb, simrank_shardplan_run and
// simrank_shardbiplan_run) with a scripted fake, on the host alone: make -C simrank_amd/csrc loop_check
// (AddressSanitizer + UBSan).  Every combination of
//
//     iterations 0 .. 5  x  eps {0.5, 1.0, 1.5, NaN}  x  first zero count at update 1 .. 5 or never
//     x  callback {null, never stops, stops at index 0 .. 5}  x  speculate {off, on}
//     x  failing call {none, queueing update j, counting update j : j = 1 .. 5, dropping the speculative update}
//
// is compared with `spec` below — the reference's loop written out plainly, without speculation — in updates_done,
// converged_at, the exact callback sequence, the returned code and which update is current; the fake itself asserts the
// ordering rules (when an update may be queued, that a counter slot is read before it is written again, that nothing is
// called after a failure).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "loop.h"

namespace {

constexpr int kQueueFailed = 7, kCountFailed = 9, kDropFailed = 11;

struct Case {
    int32_t iterations = 0;
    double eps = 0.5;
    int first_zero = 0;       // c_k == 0 at this update (0: never)
    int callback = 0;         // 0: null, 1: never stops, 2 + i: nonzero at loop index i
    bool speculate = false;
    int fail_queue = 0;       // queueing this update fails (0: none)
    int fail_count = 0;       // counting this update fails (0: none)
    bool fail_drop = false;   // dropping the speculative update fails
};

using Calls = std::vector<std::pair<int32_t, int32_t>>;

struct Outcome {
    int32_t done = 0, conv = -1;
    int rc = 0;
    Calls calls;
};

[[noreturn]] void fail(const Case& c, const char* what) {
    std::fprintf(stderr,
                 "loop_check: %s\n  iterations %d eps %g first_zero %d callback %d speculate %d fail_queue %d fail_count %d fail_drop %d\n",
                 what, c.iterations, c.eps, c.first_zero, c.callback, (int)c.speculate, c.fail_queue, c.fail_count, (int)c.fail_drop);
    std::exit(1);
}

struct Listener {
    const Case* c;
    Calls calls;
    bool* failed;
};

int32_t on_progress(void* user, int32_t k, int32_t converged) {
    Listener* l = static_cast<Listener*>(user);
    if (*l->failed) fail(*l->c, "progress called after a failure");
    l->calls.emplace_back(k, converged);
    return l->c->callback >= 2 && k == l->c->callback - 2 ? 1 : 0;      // (also where converged = 1: must be ignored)
}

// The specification: SimRank.py's loop as it stands — test, progress, update —, one update at a time.  `speculate`
// enters only in WHEN a failing queue call is met — update k + 1 is queued before c_k is read — and in the drop of that
// update when the loop ends at an index k >= 1, whose failure is the returned code.
Outcome spec(const Case& c) {
    Outcome e;
    auto tell = [&](int32_t k, int32_t converged) {
        if (c.callback == 0) return false;
        e.calls.emplace_back(k, converged);
        return c.callback >= 2 && k == c.callback - 2;
    };
    bool dropped = false;
    for (int32_t k = 0; k < c.iterations; ++k) {
        if (k == 0) {
            if (!(1.0 > c.eps)) { e.conv = 0; (void)tell(0, 1); break; }
        } else {
            if (c.speculate && c.fail_queue == k + 1) { e.rc = kQueueFailed; return e; }
            if (c.fail_count == k) { e.rc = kCountFailed; return e; }
            if (c.first_zero == k) { e.conv = k; (void)tell(k, 1); dropped = c.speculate; break; }
        }
        if (tell(k, 0)) { dropped = c.speculate && k >= 1; break; }
        if ((k == 0 || !c.speculate) && c.fail_queue == k + 1) { e.rc = kQueueFailed; return e; }
        e.done = k + 1;
    }
    if (dropped && c.fail_drop) e.rc = kDropFailed;
    return e;
}

struct Fake {
    const Case& c;
    bool failed = false;
    int queued = 0, adopted = 0, dropped = 0;
    int read_upto = 0;                        // counts read: c_1 .. c_read_upto
    int slot_update[2] = {0, 0};              // the update whose count a slot holds
    bool slot_read[2] = {true, true};
    int last_slot = -1;

    void alive(const char* what) const { if (failed) fail(c, what); }
    void need(bool ok, const char* what) const { if (!ok) fail(c, what); }

    int queue(int slot) {
        alive("queue called after a failure");
        const int j = queued + 1;             // updates are queued in order 1, 2, ...
        need(slot == 0 || slot == 1, "slot out of range");
        need(slot != last_slot, "two consecutive updates share a slot");
        need(slot_read[slot], "a slot is overwritten before it was read");
        need(j <= c.iterations, "more updates queued than iterations");
        need(adopted == j - 1, "an update is queued more than one ahead");
        if (c.speculate) need(read_upto == (j >= 2 ? j - 2 : 0), "speculation lost: update k + 1 queued after c_k was read");
        else need(adopted == j - 1 && read_upto == j - 1, "update k + 1 queued before c_k was read, without speculation");
        queued = j;
        last_slot = slot;
        slot_update[slot] = j;
        slot_read[slot] = false;
        if (c.fail_queue == j) { failed = true; return kQueueFailed; }
        return 0;
    }
    int count(int slot, bool* zero) {
        alive("count called after a failure");
        need(slot == 0 || slot == 1, "slot out of range");
        const int k = adopted;
        need(k >= 1 && slot_update[slot] == k && !slot_read[slot], "the slot read does not hold the count of the current update");
        need(k < c.iterations, "a test after the last update");
        need(queued == (c.speculate ? k + 1 : k), "wrong number of updates queued when c_k is read");
        slot_read[slot] = true;
        read_upto = k;
        if (c.fail_count == k) { failed = true; return kCountFailed; }
        *zero = k == c.first_zero;
        return 0;
    }
    void adopt() {
        alive("adopt called after a failure");
        need(adopted < queued, "adopted an update that was never queued");
        ++adopted;
    }
    int drop() {
        alive("drop called after a failure");
        need(c.speculate && queued == adopted + 1 && dropped == 0, "drop without a speculative update");
        ++dropped;
        if (c.fail_drop) { failed = true; return kDropFailed; }
        return 0;
    }
    int current() const { return queued - dropped; }      // (a plan whose queue call itself moves on to the new iterate)
};

void run_case(const Case& c) {
    const Outcome want = spec(c);
    Fake fake{c};
    Listener l{&c, {}, &fake.failed};
    const simrank::LoopResult got = simrank::run_loop(fake, c.iterations, c.eps, c.speculate,
                                                      c.callback ? on_progress : nullptr, c.callback ? &l : nullptr);
    if (got.rc != want.rc) fail(c, "returned code");
    if (l.calls != want.calls) fail(c, "callback sequence");
    if (got.done != want.done) fail(c, "updates_done");
    if (got.rc) return;
    if (got.conv != want.conv) fail(c, "converged_at");
    if (fake.adopted != got.done || fake.current() != got.done) fail(c, "the current iterate is not update `done`");
    if (!c.speculate && fake.queued != got.done) fail(c, "more than `done` updates queued without speculation");
}

}  // namespace

int main() {
    const double epss[4] = {0.5, 1.0, 1.5, std::nan("")};
    long cases = 0;
    Case c;
    for (c.iterations = 0; c.iterations <= 5; ++c.iterations)
        for (double eps : epss)
            for (c.first_zero = 0; c.first_zero <= 5; ++c.first_zero)
                for (c.callback = 0; c.callback <= 7; ++c.callback)
                    for (int spec_on = 0; spec_on < 2; ++spec_on)
                        for (int f = 0; f <= 11; ++f) {
                            c.eps = eps;
                            c.speculate = spec_on != 0;
                            c.fail_queue = f >= 1 && f <= 5 ? f : 0;
                            c.fail_count = f >= 6 && f <= 10 ? f - 5 : 0;
                            c.fail_drop = f == 11;
                            run_case(c);
                            ++cases;
                        }
    std::printf("loop_check: %ld cases passed\n", cases);
    return 0;
}
