// The two device steps of a k-medoids alternation on an iterate that stays where it lies (include/simrank_kmedoids.h,
// libsimrank_kmedoids.so): every node to the medoid whose row likes it best, and every cluster's medoid to the member
// with the largest `own`.
//
//     assign  K medoid rows against all the block's columns, shaped by its READS as sets.hip's score kernel is: a
//             workgroup owns 1024 consecutive columns, a lane 4 of them, which are 16 contiguous bytes of an f32 row or
//             panel (8 of a binary16 panel, 32 of a float64 row): one vector load per medoid row, kUnroll rows' loads
//             issued before the first is consumed.  A lane keeps per column the best (value, j) so far, the value at
//             j == its current cluster and, where the column is a medoid's own node, that medoid and its value: all in
//             registers, a strict `>` in double so that the first j wins a tie.  The medoid list is uniform over the
//             workgroup and comes through scalar loads.  No LDS, no floating-point atomics; `moved` is one integer
//             atomic per wave.
//     pick    one wave per cluster walks its list with a stride of 64 over 8-byte values; each lane keeps the (largest
//             own, earliest list index) it saw, a butterfly reduces in the order (own descending, index ascending), and
//             lane 0 compares the incumbent last, with the strict rule.
#include "simrank_kmedoids.h"

#define COMPANION_ERR_INVALID SIMRANK_KMEDOIDS_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_KMEDOIDS_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_KMEDOIDS_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_KMEDOIDS_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_KMEDOIDS_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_KMEDOIDS_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int kPerThread = 4;                              // columns of one lane
constexpr int kChunk = kThreads * kPerThread;              // columns of one workgroup
constexpr int kUnroll = 8;                                 // medoid rows whose loads are in flight together
static_assert(kChunk == SIMRANK_KMEDOIDS_CHUNK, "the header's chunk is the kernel's");

__device__ inline double nan_f64() { return __longlong_as_double(0x7ff8000000000000LL); }

// The stored bits of four consecutive columns c .. c + 3 (c a multiple of 4) of row r: 16 / 8 / 32 contiguous bytes.
template <int L> struct Quad { float4 x; };
template <> struct Quad<PANEL_F16> { uint2 x; };
template <> struct Quad<ROWMAJOR_F64> { double2 a, b; };

template <int L>
__device__ __forceinline__ Quad<L> load_quad(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c) {
    Quad<L> q;
    const int64_t at = offset_of<L>(stride, r, c);
    if constexpr (L == PANEL_F16) {
        q.x = *reinterpret_cast<const uint2*>(static_cast<const __half*>(S) + at);
    } else if constexpr (L == ROWMAJOR_F64) {
        const double2* p = reinterpret_cast<const double2*>(static_cast<const double*>(S) + at);
        q.a = p[0], q.b = p[1];
    } else {
        q.x = *reinterpret_cast<const float4*>(static_cast<const float*>(S) + at);
    }
    return q;
}

// ... widened as companion.h's `load` widens one element
template <int L>
__device__ __forceinline__ void widen(const Quad<L>& q, double (&v)[kPerThread]) {
    if constexpr (L == PANEL_F16) {
        union {
            uint2 bits;
            __half h[4];
        } x;
        x.bits = q.x;
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) v[i] = (double)(__half2float(x.h[i]) * kHalfScale);
    } else if constexpr (L == ROWMAJOR_F64) {
        v[0] = q.a.x, v[1] = q.a.y, v[2] = q.b.x, v[3] = q.b.y;
    } else {
        v[0] = (double)q.x.x, v[1] = (double)q.x.y, v[2] = (double)q.x.z, v[3] = (double)q.x.w;
    }
}

// What a lane knows of its four columns.
struct Columns {
    double best_v[kPerThread], cur_v[kPerThread], own_v[kPerThread];
    int32_t best_j[kPerThread];        // the first j in the order (v descending, j ascending); -1: no candidate yet
    int32_t cur[kPerThread];           // the column's current cluster; -1: none
    int32_t own_j[kPerThread];         // the first medoid whose own node the column is; -1: none

    // medoid j holds v[i] in column i; `d` is its own column counted from the lane's first
    __device__ __forceinline__ void take(int32_t j, const double (&v)[kPerThread], int64_t d) {
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) {
            const double x = v[i];
            if (x == x && (best_j[i] < 0 || x > best_v[i])) {
                best_v[i] = x;
                best_j[i] = j;
            }
            if (j == cur[i]) cur_v[i] = x;
            if (d == i && own_j[i] < 0) {
                own_j[i] = j;
                own_v[i] = x;
            }
        }
    }
};

// VEC: every quad of a full lane is one aligned vector load.  Otherwise, and in the lane that holds the block's last
// columns, element by element.
template <int L, bool VEC>
__global__ __launch_bounds__(kThreads) void assign_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                          int64_t n_cols, const int32_t* __restrict__ med_row,
                                                          const int32_t* __restrict__ med_col, int32_t K,
                                                          const int32_t* __restrict__ current,
                                                          int32_t* __restrict__ cluster, double* __restrict__ value,
                                                          unsigned* __restrict__ moved) {
    const int64_t j0 = blockIdx.x * int64_t(kChunk) + int64_t(threadIdx.x) * kPerThread;
    const double nan = nan_f64();
    Columns col;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        col.best_v[i] = 0.0, col.best_j[i] = -1, col.cur_v[i] = nan, col.own_v[i] = nan, col.own_j[i] = -1;
        int32_t c = -1;
        if (current && j0 + i < n_cols) c = current[j0 + i];
        col.cur[i] = (c >= 0 && c < K) ? c : -1;
    }

    if (VEC && j0 + kPerThread <= n_cols) {
        int32_t j = 0;
        for (; j + kUnroll <= K; j += kUnroll) {
            Quad<L> x[kUnroll];
            bool ok[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int64_t r = med_row[j + u];
                ok[u] = r >= 0 && r < n_rows;
                x[u] = load_quad<L>(S, stride, ok[u] ? r : 0, j0);         // (row 0 exists: n_rows > 0 where a lane is full)
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                double v[kPerThread];
                widen<L>(x[u], v);
#pragma unroll
                for (int i = 0; i < kPerThread; ++i) v[i] = ok[u] ? v[i] : nan;
                col.take(j + u, v, int64_t(med_col[j + u]) - j0);
            }
        }
        for (; j < K; ++j) {
            const int64_t r = med_row[j];
            const bool ok = r >= 0 && r < n_rows;
            double v[kPerThread];
            widen<L>(load_quad<L>(S, stride, ok ? r : 0, j0), v);
#pragma unroll
            for (int i = 0; i < kPerThread; ++i) v[i] = ok ? v[i] : nan;
            col.take(j, v, int64_t(med_col[j]) - j0);
        }
    } else if (j0 < n_cols) {
        for (int32_t j = 0; j < K; ++j) {
            const int64_t r = med_row[j];
            const bool ok = r >= 0 && r < n_rows;
            double v[kPerThread];
#pragma unroll
            for (int i = 0; i < kPerThread; ++i) v[i] = (ok && j0 + i < n_cols) ? elem<L>(S, stride, r, j0 + i) : nan;
            col.take(j, v, int64_t(med_col[j]) - j0);
        }
    }

    int n_moved = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        if (j0 + i >= n_cols) continue;
        int32_t c;
        double v;
        if (col.own_j[i] >= 0) {                                           // a medoid's own node
            c = col.own_j[i], v = col.own_v[i];
        } else if (col.cur[i] >= 0) {                                      // the stay rule
            const bool move = col.best_j[i] >= 0 && (col.best_v[i] > col.cur_v[i] || col.cur_v[i] != col.cur_v[i]);
            c = move ? col.best_j[i] : col.cur[i], v = move ? col.best_v[i] : col.cur_v[i];
        } else {
            const bool any = col.best_j[i] >= 0;
            c = any ? col.best_j[i] : 0, v = any ? col.best_v[i] : nan;
        }
        cluster[j0 + i] = c;
        value[j0 + i] = v;
        n_moved += c != col.cur[i];                                        // (no current: -1, which no cluster is)
    }
    if (moved) {                                                           // (uniform: every lane of the wave is here)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n_moved += __shfl_xor(n_moved, d);
        if ((threadIdx.x & 63) == 0 && n_moved) atomicAdd(moved, (unsigned)n_moved);
    }
}

__global__ __launch_bounds__(kThreads) void pick_kernel(const double* __restrict__ own, int64_t n_rows,
                                                        const int32_t* __restrict__ col_pos,
                                                        const int64_t* __restrict__ group_ptr, int32_t K,
                                                        int32_t* __restrict__ med_row, double* __restrict__ cohesion,
                                                        unsigned* __restrict__ changed) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (blockIdx.x * int64_t(kThreads) + threadIdx.x) >> 6;
    if (j >= K) return;                                                    // (the whole wave)
    const int64_t lo = group_ptr[j], hi = group_ptr[j + 1];
    double best_v = 0.0;
    int64_t best_e = -1;                                                   // list index from `lo`; -1: no candidate
    for (int64_t e = lane; e < hi - lo; e += 64) {
        const int32_t p = col_pos[lo + e];
        if (uint64_t(uint32_t(p)) >= uint64_t(n_rows)) continue;
        const double v = own[p];
        if (v == v && (best_e < 0 || v > best_v)) {                        // (indices ascend in a lane: the first of a tie stays)
            best_v = v;
            best_e = e;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(best_v, d);
        const int64_t oe = __shfl_xor(best_e, d);
        if (oe >= 0 && (best_e < 0 || ov > best_v || (ov == best_v && oe < best_e))) {
            best_v = ov;
            best_e = oe;
        }
    }
    if (lane != 0) return;
    const int32_t m = med_row[j];
    const double mine = uint64_t(uint32_t(m)) < uint64_t(n_rows) ? own[m] : nan_f64();
    if (best_e >= 0 && (best_v > mine || mine != mine)) {
        med_row[j] = col_pos[lo + best_e];
        cohesion[j] = best_v;
        if (changed) atomicAdd(changed, 1u);
    } else {
        cohesion[j] = hi > lo ? mine : nan_f64();
    }
}

}  // namespace

extern "C" {

int simrank_kmedoids_version(void) { return SIMRANK_KMEDOIDS_VERSION; }

const char* simrank_kmedoids_last_error(void) { return g_error.c_str(); }

int simrank_kmedoids_assign(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                            const int32_t* med_row, const int32_t* med_col, int32_t K, const int32_t* current,
                            int32_t* cluster, double* value, uint32_t* moved, void* stream) {
    const int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    const uintptr_t p = reinterpret_cast<uintptr_t>(S);
    const unsigned size = layout == ROWMAJOR_F64 ? 8 : layout == PANEL_F16 ? 2 : 4;
    REQUIRE(p % size == 0, "S must start on a multiple of its element's size (%u bytes)", size);
    REQUIRE(K >= 1, "K must be at least 1 (got %d)", (int)K);
    REQUIRE(med_row && med_col, "med_row or med_col is NULL");
    REQUIRE(n_cols == 0 || (cluster && value), "cluster or value is NULL");
    if (n_cols == 0) return SIMRANK_KMEDOIDS_OK;
    const bool vec = n_rows > 0 && quad_vector_loads(S, layout, stride);
    const dim3 grid((unsigned)((n_cols + kChunk - 1) / kChunk));
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        if (vec)
            hipLaunchKernelGGL((assign_kernel<L, true>), grid, dim3(kThreads), 0, st, S, stride, n_rows, n_cols, med_row,
                               med_col, K, current, cluster, value, moved);
        else
            hipLaunchKernelGGL((assign_kernel<L, false>), grid, dim3(kThreads), 0, st, S, stride, n_rows, n_cols, med_row,
                               med_col, K, current, cluster, value, moved);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_KMEDOIDS_OK;
}

int simrank_kmedoids_pick(const double* own, int64_t n_rows, const int32_t* col_pos, const int64_t* group_ptr, int32_t K,
                          int32_t* med_row, double* cohesion, uint32_t* changed, void* stream) {
    REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31), "bad number of rows %lld", (long long)n_rows);
    REQUIRE(K >= 1, "K must be at least 1 (got %d)", (int)K);
    REQUIRE(own || n_rows == 0, "own is NULL");
    REQUIRE(col_pos && group_ptr, "col_pos or group_ptr is NULL");
    REQUIRE(med_row && cohesion, "med_row or cohesion is NULL");
    const unsigned grid = (unsigned)((int64_t(K) + kThreads / 64 - 1) / (kThreads / 64));
    hipLaunchKernelGGL(pick_kernel, dim3(grid), dim3(kThreads), 0, as_stream(stream), own, n_rows, col_pos, group_ptr, K,
                       med_row, cohesion, changed);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_KMEDOIDS_OK;
}

}  // extern "C"
