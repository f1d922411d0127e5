// A clustering of an iterate scored where the iterate lies (include/simrank_groups.h, libsimrank_groups.so): the mean
// similarity of every node to every group of a labelling, and per node its own group's mean, the best other mean and
// that group.
//
// One workgroup per block row.  It walks the groups in chunks of 256, one group per thread, and a thread ends every
// chunk with the (row, group) mean of its group, however the sum was made:
//     a list of at most 8 positions     by the thread itself, in list order (the singleton end: K = N costs a lane a group)
//     up to 1023 positions              by the thread's wave, one such group after the other: lane l adds the members
//                                       l, l + 64, ... into four running sums, a butterfly over the lanes adds those
//     longer                            by the workgroup in the same way with a stride of 256, the four waves' sums added
//                                       in wave order
// so the order of a sum's additions depends on the list's length alone, and nothing is accumulated in memory: there are
// no atomics in this file.  The members are gathered straight from the block (one element load each, companion.h's
// `load`); a row is read once in all, scattered over the groups, and stays in the L2 while its workgroup runs.  Each
// thread keeps the best (mean, group) of the groups it owned; one reduction per row in the total order (mean
// descending, group ascending) gives `other` and `nearest`.
#include "simrank_groups.h"

#define COMPANION_ERR_INVALID SIMRANK_GROUPS_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_GROUPS_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_GROUPS_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_GROUPS_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_GROUPS_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_GROUPS_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLaneMax = SIMRANK_GROUPS_LANE_MAX;
constexpr int kWaveMax = SIMRANK_GROUPS_WAVE_MAX;
constexpr int kMaxGrid = 1 << 20;
static_assert(kWaves == 4, "the sums of the waves are added as (0 + 1) + (2 + 3)");

__device__ inline double nan_f64() { return __longlong_as_double(0x7ff8000000000000LL); }

// Member c of row r as a double: NaN outside the block.  The caller has dealt with the row's own node.
template <int L>
__device__ inline double member(const void* __restrict__ S, int64_t stride, int64_t r, int64_t n_cols, int32_t c) {
    if (uint64_t(uint32_t(c)) >= uint64_t(n_cols)) return nan_f64();
    return (double)load<L>(S, stride, r, c);
}

// This thread's share of the list col_pos[lo .. hi): the members first, first + STEP, ... in four running sums, added
// as (0 + 1) + (2 + 3).  `lo` and `hi` are the same in every lane of the wave, so the loop is, too; `left` is the
// WAVE's number of members that are the row's own node (left out of the sum).
template <int L, int STEP>
__device__ inline double strided(const void* __restrict__ S, int64_t stride, int64_t r, int64_t n_cols,
                                 const int32_t* __restrict__ col_pos, int64_t lo, int64_t hi, int first, int32_t self,
                                 int& left) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    left = 0;
    for (int64_t e0 = lo; e0 < hi; e0 += 4 * STEP) {
        int32_t c[4];
        bool on[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t e = e0 + first + i * STEP;
            on[i] = e < hi;
            c[i] = on[i] ? col_pos[e] : 0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool me = on[i] && self >= 0 && c[i] == self;
            left += __popcll(__ballot(me));
            double v = 0.0;
            if (on[i] && !me) v = member<L>(S, stride, r, n_cols, c[i]);
            s[i] += v;
        }
    }
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// the sum over the wave's lanes, the same bits in every lane (all 64 lanes call it)
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// (v, g) comes before (bv, bg) in the order (mean descending, group ascending); g < 0 is no candidate
__device__ inline bool beats(double v, int32_t g, double bv, int32_t bg) {
    return g >= 0 && (bg < 0 || v > bv || (v == bv && g < bg));
}

template <int L>
__global__ __launch_bounds__(kThreads) void means_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                         int64_t n_cols, const int32_t* __restrict__ row_group,
                                                         const int32_t* __restrict__ row_col,
                                                         const int32_t* __restrict__ col_pos,
                                                         const int64_t* __restrict__ group_ptr, int64_t n_groups,
                                                         double* __restrict__ own, double* __restrict__ other,
                                                         int32_t* __restrict__ nearest, double* __restrict__ means,
                                                         int64_t ld_means) {
    __shared__ unsigned long long s_big[kWaves];
    __shared__ double s_sum[kWaves];
    __shared__ int s_left[kWaves];
    __shared__ double s_best_v[kWaves];
    __shared__ int32_t s_best_g[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int32_t mine = row_group[r];
        if (mine < 0) continue;                                          // (the same in every thread of the workgroup)
        const int32_t self = row_col[r];
        double best_v = 0.0;
        int32_t best_g = -1;
        for (int64_t g0 = 0; g0 < n_groups; g0 += kThreads) {
            const int64_t g = g0 + tid;
            const bool live = g < n_groups;
            const int64_t lo = live ? group_ptr[g] : 0, hi = live ? group_ptr[g + 1] : 0;
            const int64_t m = hi - lo;
            double sum = 0.0;
            int64_t left = 0;
            // a short list: this lane, in list order
            if (live && m <= kLaneMax) {
                for (int64_t e = lo; e < hi; ++e) {
                    const int32_t c = col_pos[e];
                    if (self >= 0 && c == self) ++left;
                    else sum += member<L>(S, stride, r, n_cols, c);
                }
            }
            // a list for the wave: one after the other, every lane of the wave on each
            uint64_t todo = __ballot(live && m > kLaneMax && m <= kWaveMax);
            while (todo) {                                               // (wave-uniform)
                const int src = __ffsll((unsigned long long)todo) - 1;
                todo &= todo - 1;
                const int64_t lo2 = __shfl(lo, src), hi2 = __shfl(hi, src);
                int skipped;
                const double s = wave_sum(strided<L, 64>(S, stride, r, n_cols, col_pos, lo2, hi2, lane, self, skipped));
                if (lane == src) {
                    sum = s;
                    left = skipped;
                }
            }
            // a list for the workgroup: every wave tells the others which of its groups are such
            const bool big = live && m > kWaveMax;
            const uint64_t bigs = __ballot(big);
            if (lane == 0) s_big[wave] = bigs;
            if (__syncthreads_or(big)) {                                 // (uniform over the workgroup from here on)
                unsigned long long masks[kWaves];
#pragma unroll
                for (int w = 0; w < kWaves; ++w) masks[w] = s_big[w];
#pragma unroll 1
                for (int w = 0; w < kWaves; ++w) {
                    unsigned long long todo_w = masks[w];
                    while (todo_w) {
                        const int src = __ffsll(todo_w) - 1;
                        todo_w &= todo_w - 1;
                        const int64_t gg = g0 + w * 64 + src;
                        const int64_t lo2 = group_ptr[gg], hi2 = group_ptr[gg + 1];
                        int skipped;
                        const double s = wave_sum(strided<L, kThreads>(S, stride, r, n_cols, col_pos, lo2, hi2, tid, self, skipped));
                        if (lane == 0) {
                            s_sum[wave] = s;
                            s_left[wave] = skipped;
                        }
                        __syncthreads();
                        if (tid == w * 64 + src) {
                            sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
                            left = int64_t(s_left[0]) + s_left[1] + s_left[2] + s_left[3];
                        }
                        __syncthreads();
                    }
                }
            }
            if (live) {
                const int64_t count = m - left;
                const double mean = count > 0 ? sum / double(count) : nan_f64();
                if (means) means[r * ld_means + g] = mean;
                if (g == mine) own[r] = mean;
                else if (mean == mean && (best_g < 0 || mean > best_v)) {    // (groups ascend in a thread: the first of a tie stays)
                    best_v = mean;
                    best_g = int32_t(g);
                }
            }
        }
        // the best of the workgroup
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double ov = __shfl_xor(best_v, d);
            const int32_t og = __shfl_xor(best_g, d);
            if (beats(ov, og, best_v, best_g)) {
                best_v = ov;
                best_g = og;
            }
        }
        if (lane == 0) {
            s_best_v[wave] = best_v;
            s_best_g[wave] = best_g;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kWaves; ++w)
                if (beats(s_best_v[w], s_best_g[w], best_v, best_g)) {
                    best_v = s_best_v[w];
                    best_g = s_best_g[w];
                }
            other[r] = best_g >= 0 ? best_v : nan_f64();
            nearest[r] = best_g;
        }
        __syncthreads();                                                 // (the next row writes the shared arrays again)
    }
}

}  // namespace

extern "C" {

int simrank_groups_version(void) { return SIMRANK_GROUPS_VERSION; }

const char* simrank_groups_last_error(void) { return g_error.c_str(); }

int simrank_groups_means(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                         const int32_t* row_group, const int32_t* row_col, const int32_t* col_pos, const int64_t* group_ptr,
                         int32_t n_groups, double* own, double* other, int32_t* nearest, double* means, int64_t ld_means,
                         void* stream) {
    const int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    const uintptr_t p = reinterpret_cast<uintptr_t>(S);
    const unsigned size = layout == ROWMAJOR_F64 ? 8 : layout == PANEL_F16 ? 2 : 4;
    REQUIRE(p % size == 0, "S must start on a multiple of its element's size (%u bytes)", size);
    REQUIRE(n_groups >= 1, "n_groups must be at least 1 (got %d)", (int)n_groups);
    REQUIRE(group_ptr, "group_ptr is NULL");
    REQUIRE(col_pos, "col_pos is NULL");
    REQUIRE(n_rows == 0 || (row_group && row_col), "row_group or row_col is NULL");
    REQUIRE(n_rows == 0 || (own && other && nearest), "own, other or nearest is NULL");
    REQUIRE(!means || ld_means >= n_groups, "ld_means %lld is smaller than n_groups (%d)", (long long)ld_means, (int)n_groups);
    if (n_rows == 0) return SIMRANK_GROUPS_OK;
    const int grid = (int)std::min<int64_t>(n_rows, kMaxGrid);
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL((means_kernel<L>), dim3(grid), dim3(kThreads), 0, st, S, stride, n_rows, n_cols, row_group,
                           row_col, col_pos, group_ptr, (int64_t)n_groups, own, other, nearest, means, ld_means);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_GROUPS_OK;
}

}  // extern "C"
