// Which neighbour pairs make two nodes similar (include/simrank_explain.h, libsimrank_explain.so): per pair (a, b) the
// sub-matrix S[I(a), I(b)] of an iterate that stays where it lies, its sums and its k largest contributors.
//
//     gather  one element read per element written, each in a cache line of its own in the worst case.  blockIdx.x is the
//             pair, blockIdx.y strides over chunks of 1024 elements of its piece, four per lane, the four loads issued
//             before the first is consumed.  What a wave-instruction's 64 lanes have in common decides what its 64 lines
//             have in common: in a row-major block consecutive lanes take consecutive j of one i, so the lines lie in
//             one row of the block (128 KiB of an f32 row at N = 32768) and the piece is written in whole lines; in a
//             panel block whose row list is the longer one consecutive lanes take consecutive i of one j, so the lines
//             lie in ONE panel (stride x 128 bytes; a dense row list makes them neighbours there), where row-wise lanes
//             would touch up to 64 panels 4 MiB apart; the piece is then written 8 bytes per line and instruction, which
//             the L2 merges.  A panel block whose column list is the longer one is read row-wise like a row-major one:
//             its 64 consecutive j fall into few panels.  No LDS.
//     reduce  rows: a lane group of 8 .. 64 lanes (by the length of a row) per row, a butterfly inside the group; columns:
//             a workgroup per 64 columns, its eight waves take the rows i mod 8 and meet in LDS in wave order; raw: the
//             row sums again, by the first workgroup of the pair.  The order of every sum is a function of na and nb.
//     select  one workgroup per pair streams the piece once and keeps the best so far in LDS: candidates that beat the
//             k-th best are appended to a buffer (the order of arrival does not matter: the total order decides), a
//             bitonic sort of best + buffer makes room.  Keys are the value's bits made sortable and the flat index
//             i * nb + j; values are copied back from the bits.
#include "simrank_explain.h"

#define COMPANION_ERR_INVALID SIMRANK_EXPLAIN_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_EXPLAIN_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_EXPLAIN_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_EXPLAIN_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_EXPLAIN_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_EXPLAIN_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                                 // gather: loads of one lane in flight
constexpr int kChunk = kThreads * kUnroll;                 // gather: elements of one workgroup and turn
constexpr int kColThreads = 512;                           // reduce, columns: eight waves
constexpr int kColWaves = kColThreads / 64;
constexpr int kSelUnroll = 32;                             // select: elements of one lane and turn (a bit each in `pending`)
constexpr int kBlocksWanted = 16384;                       // workgroups a launch aims at when the pairs alone are fewer
constexpr int kMaxGridY = 65535;
static_assert(SIMRANK_EXPLAIN_MAX_K == 1024, "the header's largest k is the select kernel's");

__device__ inline double nan_f64() { return __longlong_as_double(0x7ff8000000000000LL); }

// What every kernel knows of its pair; `ok` is false for a pair whose piece is not na x nb (skipped).
struct Pair {
    int64_t a0, na, b0, nb, o0, total;
    bool ok;
};

__device__ inline Pair pair_of(const int64_t* __restrict__ a_ptr, const int64_t* __restrict__ b_ptr,
                               const int64_t* __restrict__ band_ptr, int64_t p) {
    Pair q;
    q.a0 = a_ptr[p], q.na = a_ptr[p + 1] - q.a0;
    q.b0 = b_ptr[p], q.nb = b_ptr[p + 1] - q.b0;
    q.o0 = band_ptr[p];
    q.ok = q.na >= 0 && q.nb >= 0 && q.na < (int64_t(1) << 31) && q.nb < (int64_t(1) << 31);
    q.total = q.ok ? q.na * q.nb : 0;
    q.ok = q.ok && band_ptr[p + 1] - q.o0 == q.total;
    return q;
}

// f / d and f % d for 0 <= f, 1 <= d < 2^31: a 32-bit division where f allows it
__device__ inline void divide(int64_t f, int64_t d, bool small, int64_t& quot, int64_t& rem) {
    if (small) {
        const uint32_t q = uint32_t(f) / uint32_t(d);
        quot = q, rem = uint32_t(f) - q * uint32_t(d);
    } else {
        quot = f / d, rem = f - quot * d;
    }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
template <int L>
__global__ __launch_bounds__(kThreads) void gather_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                          int64_t n_cols, const int32_t* __restrict__ a_pos,
                                                          const int64_t* __restrict__ a_ptr,
                                                          const int32_t* __restrict__ b_pos,
                                                          const int64_t* __restrict__ b_ptr,
                                                          const int64_t* __restrict__ band_ptr, double* __restrict__ band) {
    const Pair pr = pair_of(a_ptr, b_ptr, band_ptr, blockIdx.x);
    if (!pr.ok || pr.total == 0) return;
    // consecutive lanes take consecutive i of one j: a panel block whose row list is the longer (the denser) one
    const bool by_column = (L == PANEL_F32 || L == PANEL_F16) && pr.na >= pr.nb;
    const bool small = pr.total <= 0xffffffffLL;
    const bool any = n_rows > 0 && n_cols > 0;                             // (an empty block: every position is outside)
    const double nan = nan_f64();
    using T = typename Stored<L>::type;
    for (int64_t base = int64_t(blockIdx.y) * kChunk; base < pr.total; base += int64_t(gridDim.y) * kChunk) {
        // No load below sits behind a lane's own branch, so that the four are in flight together: a lane past the end
        // of the piece reads what the piece's last element reads and writes nothing; a position outside the block reads
        // element (0, 0), which is inside, and writes NaN.
        int64_t at[kUnroll], off[kUnroll];
        bool ok[kUnroll];
        T x[kUnroll] = {};
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t f = base + u * kThreads + threadIdx.x;
            const bool live = f < pr.total;
            int64_t i, j;
            if (by_column) divide(live ? f : pr.total - 1, pr.na, small, j, i);
            else divide(live ? f : pr.total - 1, pr.nb, small, i, j);
            at[u] = live ? i * pr.nb + j : -1;
            const int64_t r = a_pos[pr.a0 + i], c = b_pos[pr.b0 + j];
            ok[u] = any && r >= 0 && r < n_rows && c >= 0 && c < n_cols;
            off[u] = offset_of<L>(stride, ok[u] ? r : 0, ok[u] ? c : 0);
        }
        if (any) {
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) x[u] = static_cast<const T*>(S)[off[u]];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            double v;                                                      // widened as companion.h's `load` widens
            if constexpr (L == PANEL_F16) v = (double)(__half2float(x[u]) * kHalfScale);
            else v = (double)x[u];
            if (at[u] >= 0) band[pr.o0 + at[u]] = ok[u] ? v : nan;
        }
    }
}

// ---- reduce ----------------------------------------------------------------------------------------------------------------
__device__ inline bool contributes(double x) { return x == x && x != 0.0; }

__global__ __launch_bounds__(kThreads) void rows_kernel(const double* __restrict__ band, const int64_t* __restrict__ a_ptr,
                                                        const int64_t* __restrict__ b_ptr,
                                                        const int64_t* __restrict__ band_ptr, double* __restrict__ row_sum,
                                                        unsigned long long* __restrict__ contributors) {
    const Pair pr = pair_of(a_ptr, b_ptr, band_ptr, blockIdx.x);
    if (!pr.ok) return;
    const int G = pr.nb > 32 ? 64 : pr.nb > 16 ? 32 : pr.nb > 8 ? 16 : 8;       // lanes of one row
    const int R = 64 / G;                                                      // rows of one wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / G, q = lane % G;
    unsigned long long cnt = 0;
    for (int64_t i0 = (int64_t(blockIdx.y) * (kThreads / 64) + wave) * R; i0 < pr.na;
         i0 += int64_t(gridDim.y) * (kThreads / 64) * R) {
        const int64_t i = i0 + sub;
        const bool live = i < pr.na;
        double acc = 0.0;
        if (live) {
            const double* row = band + pr.o0 + i * pr.nb;
            for (int64_t j = q; j < pr.nb; j += G) {
                const double x = row[j];
                acc += x;
                cnt += contributes(x);
            }
        }
        for (int d = G >> 1; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);       // (inside the group: d < G)
        if (live && q == 0) row_sum[pr.a0 + i] = acc;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0 && cnt) atomicAdd(contributors + blockIdx.x, cnt);
}

__global__ __launch_bounds__(kColThreads) void cols_kernel(const double* __restrict__ band, const int64_t* __restrict__ a_ptr,
                                                           const int64_t* __restrict__ b_ptr,
                                                           const int64_t* __restrict__ band_ptr,
                                                           const double* __restrict__ row_sum, double* __restrict__ col_sum,
                                                           double* __restrict__ raw) {
    __shared__ double part[kColWaves][64];
    const Pair pr = pair_of(a_ptr, b_ptr, band_ptr, blockIdx.x);
    if (!pr.ok) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_strips = (pr.nb + 63) / 64;
    for (int64_t s = blockIdx.y; s < n_strips; s += gridDim.y) {
        const int64_t j = s * 64 + lane;
        const bool live = j < pr.nb;
        double acc = 0.0;
        if (live) {
            const double* col = band + pr.o0 + j;
#pragma unroll 4
            for (int64_t i = wave; i < pr.na; i += kColWaves) acc += col[i * pr.nb];
        }
        part[wave][lane] = acc;
        __syncthreads();
        if (wave == 0 && live) {
            double t = part[0][lane];
#pragma unroll
            for (int w = 1; w < kColWaves; ++w) t += part[w][lane];
            col_sum[pr.b0 + j] = t;
        }
        __syncthreads();
    }
    if (blockIdx.y == 0 && wave == 0) {                                        // raw: the sum of the row sums
        double acc = 0.0;
        for (int64_t i = lane; i < pr.na; i += 64) acc += row_sum[pr.a0 + i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) raw[blockIdx.x] = acc;
    }
}

// ---- select ----------------------------------------------------------------------------------------------------------------
constexpr uint64_t kNoKey = ~uint64_t(0);                  // an empty slot: after every real key
constexpr int64_t kNoPos = INT64_MAX;

// ascending keys = descending values; no contributor maps to kNoKey (that would be a NaN's bits)
__device__ inline uint64_t key_of(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return ~((b >> 63) ? ~b : (b | (uint64_t(1) << 63)));
}

__device__ inline double value_of(uint64_t key) {
    const uint64_t u = ~key;
    return __longlong_as_double((long long)((u >> 63) ? (u & ~(uint64_t(1) << 63)) : ~u));
}

__device__ inline bool before(uint64_t ka, int64_t pa, uint64_t kb, int64_t pb) { return ka < kb || (ka == kb && pa < pb); }

// key / pos [0, N2) ascending in (key, pos); every thread of the workgroup calls it
template <int N2>
__device__ inline void sort_all(uint64_t* key, int64_t* pos) {
    for (int size = 2; size <= N2; size <<= 1) {
        for (int st = size >> 1; st > 0; st >>= 1) {
            for (int t = threadIdx.x; t < N2 / 2; t += kThreads) {
                const int lo = 2 * t - (t & (st - 1)), hi = lo + st;
                const bool up = (lo & size) == 0;
                const uint64_t kl = key[lo], kh = key[hi];
                const int64_t pl = pos[lo], ph = pos[hi];
                if (before(kh, ph, kl, pl) == up) {
                    key[lo] = kh, key[hi] = kl;
                    pos[lo] = ph, pos[hi] = pl;
                }
            }
            __syncthreads();
        }
    }
}

// KP: slots of the best so far and of the buffer, a power of two >= k
template <int KP>
__global__ __launch_bounds__(kThreads) void select_kernel(const double* __restrict__ band, const int64_t* __restrict__ a_ptr,
                                                          const int64_t* __restrict__ b_ptr,
                                                          const int64_t* __restrict__ band_ptr, int32_t k,
                                                          int32_t* __restrict__ best_i, int32_t* __restrict__ best_j,
                                                          double* __restrict__ best_value) {
    __shared__ uint64_t key[2 * KP];
    __shared__ int64_t pos[2 * KP];
    __shared__ int count;
    const int64_t p = blockIdx.x;
    const Pair pr = pair_of(a_ptr, b_ptr, band_ptr, p);
    if (!pr.ok) return;
    for (int t = threadIdx.x; t < 2 * KP; t += kThreads) key[t] = kNoKey, pos[t] = kNoPos;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    uint64_t thr_key = kNoKey;                             // the k-th best so far (uniform)
    int64_t thr_pos = kNoPos;

    // best + buffer sorted, the buffer emptied, the threshold read again
    auto merge = [&]() {
        sort_all<2 * KP>(key, pos);
        for (int t = KP + threadIdx.x; t < 2 * KP; t += kThreads) key[t] = kNoKey, pos[t] = kNoPos;
        if (threadIdx.x == 0) count = 0;
        thr_key = key[k - 1], thr_pos = pos[k - 1];
        __syncthreads();
    };

    for (int64_t base = 0; base < pr.total; base += kThreads * kSelUnroll) {
        uint64_t mine[kSelUnroll];
        double read[kSelUnroll];
        unsigned pending = 0;
        // every load unconditional (past the end: the piece's last element, dropped below), so that none waits for a branch
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) {
            const int64_t f = base + u * kThreads + threadIdx.x;
            read[u] = band[pr.o0 + (f < pr.total ? f : pr.total - 1)];
        }
#pragma unroll
        for (int u = 0; u < kSelUnroll; ++u) {
            const int64_t f = base + u * kThreads + threadIdx.x;
            const double x = f < pr.total ? read[u] : 0.0;
            mine[u] = key_of(x);
            if (contributes(x) && before(mine[u], f, thr_key, thr_pos)) pending |= 1u << u;
        }
        for (;;) {
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u) {
                if (!(pending & (1u << u))) continue;
                const int slot = atomicAdd(&count, 1);
                if (slot >= KP) continue;                                      // (no room: waits for the merge)
                key[KP + slot] = mine[u];
                pos[KP + slot] = base + u * kThreads + threadIdx.x;
                pending &= ~(1u << u);
            }
            if (!__syncthreads_or(pending != 0)) break;
            merge();
#pragma unroll
            for (int u = 0; u < kSelUnroll; ++u)
                if ((pending & (1u << u)) && !before(mine[u], base + u * kThreads + threadIdx.x, thr_key, thr_pos))
                    pending &= ~(1u << u);
        }
        // (count <= KP here: nobody was refused in the last turn.  The buffer is sorted in only when it overflows: until
        // then the threshold is the last merge's, which lets more in and drops none of the k best)
    }
    if (count > 0) merge();                                                    // (uniform: read after the turn's barrier)
    for (int r = threadIdx.x; r < k; r += kThreads) {
        const bool any = pos[r] != kNoPos;
        int64_t i = -1, j = -1;
        if (any) divide(pos[r], pr.nb, pr.total <= 0xffffffffLL, i, j);
        best_i[p * k + r] = (int32_t)i;
        best_j[p * k + r] = (int32_t)j;
        best_value[p * k + r] = any ? value_of(key[r]) : 0.0;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline int check_pairs(const int64_t* a_ptr, const int64_t* b_ptr, const int64_t* band_ptr, int64_t n_pairs) {
    REQUIRE(n_pairs >= 0 && n_pairs < (int64_t(1) << 31), "bad number of pairs %lld", (long long)n_pairs);
    REQUIRE(a_ptr && b_ptr && band_ptr, "a_ptr, b_ptr or band_ptr is NULL");
    return 0;
}

// workgroups along y: the units of the largest pair, as long as the launch stays near kBlocksWanted
inline unsigned grid_y(int64_t units, int64_t n_pairs) {
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(kMaxGridY, kBlocksWanted / n_pairs));
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(units, cap));
}

}  // namespace

extern "C" {

int simrank_explain_version(void) { return SIMRANK_EXPLAIN_VERSION; }

const char* simrank_explain_last_error(void) { return g_error.c_str(); }

int simrank_explain_gather(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                           const int32_t* a_pos, const int64_t* a_ptr, const int32_t* b_pos, const int64_t* b_ptr,
                           const int64_t* band_ptr, int64_t n_pairs, int64_t max_terms, double* band, void* stream) {
    int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    const uintptr_t at = reinterpret_cast<uintptr_t>(S);
    const unsigned size = layout == ROWMAJOR_F64 ? 8 : layout == PANEL_F16 ? 2 : 4;
    REQUIRE(at % size == 0, "S must start on a multiple of its element's size (%u bytes)", size);
    if ((rc = check_pairs(a_ptr, b_ptr, band_ptr, n_pairs))) return rc;
    REQUIRE(max_terms >= 0, "max_terms is negative (%lld)", (long long)max_terms);
    REQUIRE(n_pairs == 0 || max_terms == 0 || (a_pos && b_pos && band), "a_pos, b_pos or band is NULL");
    if (n_pairs == 0 || max_terms == 0) return SIMRANK_EXPLAIN_OK;
    const dim3 grid((unsigned)n_pairs, grid_y((max_terms + kChunk - 1) / kChunk, n_pairs));
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL((gather_kernel<L>), grid, dim3(kThreads), 0, as_stream(stream), S, stride, n_rows, n_cols, a_pos,
                           a_ptr, b_pos, b_ptr, band_ptr, band);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_EXPLAIN_OK;
}

int simrank_explain_reduce(const double* band, const int64_t* a_ptr, const int64_t* b_ptr, const int64_t* band_ptr,
                           int64_t n_pairs, int64_t max_rows, int64_t max_cols, double* row_sum, double* col_sum, double* raw,
                           int64_t* contributors, void* stream) {
    const int rc = check_pairs(a_ptr, b_ptr, band_ptr, n_pairs);
    if (rc) return rc;
    REQUIRE(max_rows >= 0 && max_cols >= 0, "max_rows or max_cols is negative (%lld, %lld)", (long long)max_rows,
            (long long)max_cols);
    REQUIRE(n_pairs == 0 || (raw && contributors), "raw or contributors is NULL");
    const bool any = max_rows > 0 && max_cols > 0;
    REQUIRE(n_pairs == 0 || !any || (band && row_sum && col_sum), "band, row_sum or col_sum is NULL");
    REQUIRE(n_pairs == 0 || max_rows == 0 || row_sum, "row_sum is NULL");
    REQUIRE(n_pairs == 0 || max_cols == 0 || col_sum, "col_sum is NULL");
    if (n_pairs == 0) return SIMRANK_EXPLAIN_OK;
    hipStream_t st = as_stream(stream);
    HIP_CHECK(hipMemsetAsync(contributors, 0, sizeof(int64_t) * (size_t)n_pairs, st));
    const dim3 rows((unsigned)n_pairs, grid_y((max_rows + kThreads / 64 - 1) / (kThreads / 64), n_pairs));
    hipLaunchKernelGGL(rows_kernel, rows, dim3(kThreads), 0, st, band, a_ptr, b_ptr, band_ptr, row_sum,
                       reinterpret_cast<unsigned long long*>(contributors));
    HIP_CHECK(hipGetLastError());
    const dim3 cols((unsigned)n_pairs, grid_y((max_cols + 63) / 64, n_pairs));
    hipLaunchKernelGGL(cols_kernel, cols, dim3(kColThreads), 0, st, band, a_ptr, b_ptr, band_ptr, row_sum, col_sum, raw);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_EXPLAIN_OK;
}

int simrank_explain_select(const double* band, const int64_t* a_ptr, const int64_t* b_ptr, const int64_t* band_ptr,
                           int64_t n_pairs, int32_t k, int32_t* best_i, int32_t* best_j, double* best_value, void* stream) {
    const int rc = check_pairs(a_ptr, b_ptr, band_ptr, n_pairs);
    if (rc) return rc;
    REQUIRE(k >= 1 && k <= SIMRANK_EXPLAIN_MAX_K, "k must be in 1 .. %d (got %d)", SIMRANK_EXPLAIN_MAX_K, (int)k);
    REQUIRE(n_pairs == 0 || (best_i && best_j && best_value), "best_i, best_j or best_value is NULL");
    if (n_pairs == 0) return SIMRANK_EXPLAIN_OK;
    const dim3 grid((unsigned)n_pairs);
    if (k <= 256)
        hipLaunchKernelGGL((select_kernel<256>), grid, dim3(kThreads), 0, as_stream(stream), band, a_ptr, b_ptr, band_ptr, k,
                           best_i, best_j, best_value);
    else
        hipLaunchKernelGGL((select_kernel<1024>), grid, dim3(kThreads), 0, as_stream(stream), band, a_ptr, b_ptr, band_ptr, k,
                           best_i, best_j, best_value);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_EXPLAIN_OK;
}

}  // extern "C"
