// Result queries on an iterate that stays on the device (include/simrank_select.h, libsimrank_select.so): which pairs of
// nodes are at least t similar, without the N x N hand-back (the second half after top-k).
//
// Two passes over a block of the iterate, in the layout the plan stores it (f32 panels, f32 row-major shard blocks,
// fp16-held panels read in place), with the same row -> wave map:
//     count   per row, the columns c with S[r][c] >= t32 and id(c) != id(r)
//     emit    the (caller id, value) of every hit at offsets[r] + its rank in the row, from ballots and prefix counts
//             inside the wave (no atomics: one deterministic output)
// The scan of the counts into int64 offsets and the move into the caller's order (whole row segments, then a sort
// of each row by caller id on up to 16 host threads) are host code of this file.
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "simrank_select.h"

#define COMPANION_ERR_INVALID SIMRANK_SELECT_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_SELECT_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_SELECT_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_SELECT_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_SELECT_, PANEL_F16);

// One kernel for both passes and the three layouts, on the shared walk (companion.h: eight rows per wave on panels, one
// on a row-major block, four 16-byte loads in flight per lane).  A lane's columns precede those of the next lane of its
// row, so a hit's rank in its row is (hits of the row's lower lanes) + (the lane's own earlier hits): ballots and
// popcounts.
template <int LAYOUT, bool EMIT>
__global__ __launch_bounds__(kSweepThreads) void select_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                               int64_t n_cols, const int32_t* __restrict__ row_ids,
                                                               const int32_t* __restrict__ col_ids, float t32,
                                                               int32_t* __restrict__ counts,
                                                               const int64_t* __restrict__ offsets, int64_t capacity,
                                                               int32_t* __restrict__ ids_out, float* __restrict__ vals_out,
                                                               int vec) {
    using E = Elem<LAYOUT>;
    WALK_GEOMETRY(LAYOUT, n_cols);
    const uint64_t row_mask = L == 64 ? ~0ull : (0xffull << (8 * g));
    const uint64_t lower = row_mask & ((1ull << lane) - 1);          // the row's lanes before this one
    for (int64_t r0 = wave * R; r0 < n_rows; r0 += nwaves * R) {
        const int64_t r = r0 + g;
        const bool live = r < n_rows;
        const int32_t rid = live ? (row_ids ? row_ids[r] : int32_t(r)) : 0;
        int64_t pos = 0, end = 0;                // (emit) the row's next slot and where its slots end
        if (EMIT && live) {
            pos = offsets[r];
            end = offsets[r + 1] < capacity ? offsets[r + 1] : capacity;
        }
        int32_t cnt = 0;
        for (int64_t k0 = 0; k0 < n_chunks; k0 += U) {
            WALK_LOAD(LAYOUT, x, S, stride, r, live, k0, n_cols, vec)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t c0 = (k0 + u) * W + int64_t(q) * V;
                float v[V];
#pragma unroll
                for (int i = 0; i < V; ++i) v[i] = E::value(E::raw(x[u], i));
                unsigned hit = 0;
                int32_t cid[V];
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    cid[i] = 0;
                    if (live && c0 + i < n_cols && v[i] >= t32) {
                        // (ids are read only where the value passed: the diagonal, and the ids the emit pass writes)
                        cid[i] = col_ids ? col_ids[c0 + i] : int32_t(c0 + i);
                        if (cid[i] != rid) hit |= 1u << i;
                    }
                }
                if (!EMIT) {
                    cnt += __builtin_popcount(hit);
                    continue;
                }
                if (!__ballot(hit != 0)) continue;           // (wave-uniform: most chunks hold no hit)
                int64_t before = 0, in_row = 0;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const uint64_t m = __ballot((hit >> i) & 1u);
                    before += __popcll(m & lower);
                    in_row += __popcll(m & row_mask);
                }
                int64_t slot = pos + before;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if ((hit >> i) & 1u) {
                        if (slot >= 0 && slot < end) {
                            ids_out[slot] = cid[i];
                            vals_out[slot] = v[i];
                        }
                        ++slot;
                    }
                }
                pos += in_row;
            }
        }
        if (!EMIT) {
#pragma unroll
            for (int off = L / 2; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
            if (live && q == 0) counts[r] = cnt;
        }
    }
}

// a swept block (companion.h) with select's own rules on top: at least one row, no float64 iterate, a threshold > 0
int plan_select(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols, float t32, Launch* l) {
    REQUIRE(known_layout(layout) && layout != ROWMAJOR_F64, "unknown layout %d", (int)layout);
    REQUIRE(n_rows > 0, "bad block shape %lld x %lld", (long long)n_rows, (long long)n_cols);
    const int rc = plan_launch(S, layout, stride, n_rows, n_cols, false, l);
    if (rc) return rc;
    REQUIRE(t32 > 0.f, "the threshold must be > 0");
    return SIMRANK_SELECT_OK;
}

template <bool EMIT>
int launch(const Launch& l, const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
           const int32_t* row_ids, const int32_t* col_ids, float t32, int32_t* counts, const int64_t* offsets,
           int64_t capacity, int32_t* ids_out, float* vals_out, void* stream) {
    with_layout(layout, [&](auto L) {
        if constexpr (L != ROWMAJOR_F64)
            hipLaunchKernelGGL((select_kernel<L, EMIT>), dim3(l.grid), dim3(kSweepThreads), 0, as_stream(stream), S, stride,
                               n_rows, n_cols, row_ids, col_ids, t32, counts, offsets, capacity, ids_out, vals_out, l.vec);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_SELECT_OK;
}

// CPUs this process may use: its affinity mask, capped by a cgroup CPU quota when there is one (as handback.hip's)
int64_t cpu_share() {
    int64_t n = std::max<int64_t>(1, (int64_t)std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::max<int64_t>(1, CPU_COUNT(&set));
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char a[64] = "", b[64] = "";
        const int got = std::fscanf(f, "%63s %63s", a, b);
        std::fclose(f);
        if (got == 2 && std::strcmp(a, "max") != 0 && std::atof(b) > 0)
            n = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)std::ceil(std::atof(a) / std::atof(b))));
    }
    return n;
}

}  // namespace

extern "C" {

int simrank_select_version(void) { return SIMRANK_SELECT_VERSION; }

const char* simrank_select_last_error(void) { return g_error.c_str(); }

int simrank_select_threshold_f32(double t, float* t32) {
    REQUIRE(t32, "t32 is NULL");
    REQUIRE(std::isfinite(t) && t > 0.0, "the threshold must be a finite number > 0 (got %g)", t);
    // (float)t is the nearest float: the smallest float >= t is it or the next one up (t > FLT_MAX: +inf)
    float f = (float)t;
    if ((double)f < t) f = std::nextafter(f, HUGE_VALF);
    else if (f > 0.f && (double)std::nextafter(f, 0.f) >= t) f = std::nextafter(f, 0.f);
    *t32 = f;
    return SIMRANK_SELECT_OK;
}

int simrank_select_count(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                         const int32_t* row_ids, const int32_t* col_ids, float t32, int32_t* counts, void* stream) {
    Launch l;
    const int rc = plan_select(S, layout, stride, n_rows, n_cols, t32, &l);
    if (rc) return rc;
    REQUIRE(counts, "counts is NULL");
    if (n_cols == 0) {
        HIP_CHECK(hipMemsetAsync(counts, 0, size_t(n_rows) * sizeof(int32_t), as_stream(stream)));
        return SIMRANK_SELECT_OK;
    }
    return launch<false>(l, S, layout, stride, n_rows, n_cols, row_ids, col_ids, t32, counts, nullptr, 0, nullptr, nullptr,
                         stream);
}

int simrank_select_offsets(const int32_t* counts, int64_t n_rows, int64_t* offsets, int64_t* total) {
    REQUIRE(counts && offsets && n_rows >= 0, "bad offsets arguments");
    int64_t s = 0;
    offsets[0] = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        REQUIRE(counts[r] >= 0, "count %d of row %lld is negative", (int)counts[r], (long long)r);
        s += counts[r];
        offsets[r + 1] = s;
    }
    if (total) *total = s;
    return SIMRANK_SELECT_OK;
}

int simrank_select_emit(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                        const int32_t* row_ids, const int32_t* col_ids, float t32, const int64_t* offsets, int64_t capacity,
                        int32_t* ids_out, float* vals_out, void* stream) {
    Launch l;
    const int rc = plan_select(S, layout, stride, n_rows, n_cols, t32, &l);
    if (rc) return rc;
    REQUIRE(offsets && capacity >= 0 && (capacity == 0 || (ids_out && vals_out)), "bad emit arguments");
    if (n_cols == 0 || capacity == 0) return SIMRANK_SELECT_OK;
    return launch<true>(l, S, layout, stride, n_rows, n_cols, row_ids, col_ids, t32, nullptr, offsets, capacity, ids_out,
                        vals_out, stream);
}

int simrank_select_merge(int32_t n_pieces, const int64_t* const* offsets, const int32_t* const* ids,
                         const float* const* vals, int64_t n_rows, const int32_t* row_order, int64_t* out_offsets,
                         int32_t* out_ids, float* out_vals, int32_t threads) {
    REQUIRE(n_pieces > 0 && offsets && ids && vals && n_rows >= 0 && (row_order || !n_rows) && out_offsets,
                "bad merge arguments");
    int64_t total = 0;
    for (int32_t p = 0; p < n_pieces; ++p) {
        REQUIRE(offsets[p] && offsets[p][0] == 0, "piece %d: offsets must start at 0", (int)p);
        for (int64_t r = 0; r < n_rows; ++r)
            REQUIRE(offsets[p][r + 1] >= offsets[p][r], "piece %d: offsets decrease at row %lld", (int)p, (long long)r);
        REQUIRE(offsets[p][n_rows] == 0 || (ids[p] && vals[p]), "piece %d: ids or values are NULL", (int)p);
        total += offsets[p][n_rows];
    }
    REQUIRE(total == 0 || (out_ids && out_vals), "out_ids or out_vals is NULL");
    // row lengths in the caller's order, then their scan
    std::vector<char> seen((size_t)n_rows, 0);
    for (int64_t r = 0; r < n_rows; ++r) {
        const int32_t a = row_order[r];
        REQUIRE(a >= 0 && a < n_rows && !seen[(size_t)a], "row_order is not a permutation of 0 .. %lld",
                    (long long)n_rows - 1);
        seen[(size_t)a] = 1;
        int64_t len = 0;
        for (int32_t p = 0; p < n_pieces; ++p) len += offsets[p][r + 1] - offsets[p][r];
        out_offsets[a + 1] = len;
    }
    out_offsets[0] = 0;
    for (int64_t a = 0; a < n_rows; ++a) out_offsets[a + 1] += out_offsets[a];
    // whole segments into place, then each row sorted by id (ids are distinct in a row: (id, value bits) as one key)
    constexpr int64_t kRows = 256;
    const int64_t n_blocks = (n_rows + kRows - 1) / kRows;
    const int64_t want = threads > 0 ? threads : 16;
    const int64_t nt = std::max<int64_t>(1, std::min<int64_t>({want, 16, cpu_share(), n_blocks,
                                                                 std::max<int64_t>(1, total >> 16)}));
    std::atomic<int64_t> next{0};
    std::atomic<int> bad{0};
    auto crew = [&]() {
        std::vector<uint64_t> keys;
        for (int64_t b; (b = next.fetch_add(1)) < n_blocks;) {
            for (int64_t r = b * kRows; r < std::min(n_rows, (b + 1) * kRows); ++r) {
                const int64_t dst = out_offsets[row_order[r]];
                keys.clear();
                for (int32_t p = 0; p < n_pieces; ++p)
                    for (int64_t i = offsets[p][r]; i < offsets[p][r + 1]; ++i) {
                        uint32_t bits;
                        std::memcpy(&bits, vals[p] + i, 4);
                        keys.push_back((uint64_t(uint32_t(ids[p][i])) << 32) | bits);
                    }
                std::sort(keys.begin(), keys.end());
                for (size_t i = 0; i < keys.size(); ++i) {
                    if (i && (keys[i] >> 32) == (keys[i - 1] >> 32)) bad.store(1);
                    out_ids[dst + (int64_t)i] = int32_t(keys[i] >> 32);
                    const uint32_t bits = uint32_t(keys[i]);
                    std::memcpy(out_vals + dst + (int64_t)i, &bits, 4);
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int64_t t = 1; t < nt; ++t) pool.emplace_back(crew);
    crew();
    for (auto& t : pool) t.join();
    REQUIRE(!bad.load(), "a row holds the same id twice");
    return SIMRANK_SELECT_OK;
}

}  // extern "C"
