// The two device steps of greedy facility location on an iterate that stays where it lies (include/simrank_exemplars.h,
// libsimrank_exemplars.so): the marginal gain of listed rows against the running column maxima `cover`, and a picked
// row applied to `cover`.
//
//     gains   one workgroup of 256 threads per LISTED row (the rows are scattered, so this is not the eight-consecutive-
//             rows walk of companion.h's WALK_LOAD).  Thread t owns the quads t, t + 256, ... of the row: four
//             consecutive columns, 16 contiguous bytes of an f32 row or panel (8 of a binary16 panel, 32 of a float64
//             row), one vector load each where companion.h's quad_vector_loads allows and `cover` starts on 16 bytes,
//             element by element otherwise and in the row's last, partial quad.  In the panel layouts a lane group of 8
//             (16 for binary16) reads the row's 128-byte segment of one panel and a wave reads 8 (4) panels of the SAME
//             row; row-major, a wave reads 1 KiB of the row.  The row's loads are non-temporal: it is read once, while
//             the 32 bytes of `cover` per quad are read again by every workgroup and should stay in the L2.  kUnroll
//             quads' loads are issued before the first is consumed.  A thread adds column 4 q + i into its running sum
//             i; the four sums, the butterfly over the wave and the four waves are added in the order the header
//             states, which depends on n_cols alone.  32 bytes of LDS, no atomics.
//     cover   one thread per column: it keeps the column's cover in a register and walks the list in order (the list
//             is uniform over the workgroup), so the rows apply as if one after the other; a wave counts the columns a
//             row raised with a ballot and adds them with one integer atomic.
#include "simrank_exemplars.h"

#define COMPANION_ERR_INVALID SIMRANK_EXEMPLARS_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_EXEMPLARS_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_EXEMPLARS_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_EXEMPLARS_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_EXEMPLARS_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_EXEMPLARS_, ROWMAJOR_F64);

constexpr int kThreads = SIMRANK_EXEMPLARS_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = 4;                              // columns of one quad
constexpr int kChunk = kThreads * kPerThread;              // columns the workgroup covers in one pass
constexpr int kUnroll = 4;                                 // passes whose loads are in flight together
constexpr int kGridCap = SIMRANK_EXEMPLARS_GRID_CAP;
static_assert(kWaves == 4, "the sums of the waves are added as (0 + 1) + (2 + 3)");

typedef float v4f32 __attribute__((ext_vector_type(4)));
typedef double v2f64 __attribute__((ext_vector_type(2)));
typedef unsigned v2u32 __attribute__((ext_vector_type(2)));

__device__ inline double nan_f64() { return __longlong_as_double(0x7ff8000000000000LL); }

// The stored bits of the four consecutive columns c .. c + 3 (c a multiple of 4) of row r, read past the caches' keep
// list, and their values as companion.h's `load` widens one element.
template <int L> struct Quad { v4f32 x; };
template <> struct Quad<PANEL_F16> { v2u32 x; };
template <> struct Quad<ROWMAJOR_F64> { v2f64 a, b; };

template <int L>
__device__ __forceinline__ Quad<L> load_quad(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c) {
    Quad<L> q;
    const int64_t at = offset_of<L>(stride, r, c);
    if constexpr (L == PANEL_F16) {
        q.x = __builtin_nontemporal_load(reinterpret_cast<const v2u32*>(static_cast<const __half*>(S) + at));
    } else if constexpr (L == ROWMAJOR_F64) {
        const v2f64* p = reinterpret_cast<const v2f64*>(static_cast<const double*>(S) + at);
        q.a = __builtin_nontemporal_load(p), q.b = __builtin_nontemporal_load(p + 1);
    } else {
        q.x = __builtin_nontemporal_load(reinterpret_cast<const v4f32*>(static_cast<const float*>(S) + at));
    }
    return q;
}

template <int L>
__device__ __forceinline__ void widen(const Quad<L>& q, double (&v)[kPerThread]) {
    if constexpr (L == PANEL_F16) {
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) {
            const unsigned short h = (unsigned short)(q.x[i >> 1] >> (16 * (i & 1)));
            v[i] = (double)(float(__builtin_bit_cast(_Float16, h)) * kHalfScale);
        }
    } else if constexpr (L == ROWMAJOR_F64) {
        v[0] = q.a[0], v[1] = q.a[1], v[2] = q.b[0], v[3] = q.b[1];
    } else {
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) v[i] = (double)q.x[i];
    }
}

// term(r, c): one subtraction where the element is above the cover, +0.0 otherwise (a NaN element compares false)
__device__ __forceinline__ double term(double v, double cov) { return v > cov ? v - cov : 0.0; }

// VEC: every whole quad is one aligned vector load and `cover` starts on 16 bytes.
template <int L, bool VEC>
__global__ __launch_bounds__(kThreads) void gains_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                         int64_t n_cols, const int32_t* __restrict__ rows, int64_t n_list,
                                                         const double* __restrict__ cover, double* __restrict__ gain) {
    __shared__ double s_wave[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t i = blockIdx.x; i < n_list; i += gridDim.x) {
        const int64_t r = rows ? int64_t(rows[i]) : i;
        if (r < 0 || r >= n_rows) {                                       // (the same in every thread of the workgroup)
            if (tid == 0) gain[i] = nan_f64();
            continue;
        }
        double s[kPerThread] = {0.0, 0.0, 0.0, 0.0};
        int64_t c0 = int64_t(tid) * kPerThread;
        if constexpr (VEC) {
            for (; c0 + int64_t(kUnroll - 1) * kChunk + kPerThread <= n_cols; c0 += int64_t(kUnroll) * kChunk) {
                Quad<L> x[kUnroll];
                v2f64 ca[kUnroll], cb[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int64_t c = c0 + int64_t(u) * kChunk;
                    x[u] = load_quad<L>(S, stride, r, c);
                    const v2f64* p = reinterpret_cast<const v2f64*>(cover + c);
                    ca[u] = p[0], cb[u] = p[1];
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    double v[kPerThread];
                    widen<L>(x[u], v);
                    s[0] += term(v[0], ca[u][0]), s[1] += term(v[1], ca[u][1]);
                    s[2] += term(v[2], cb[u][0]), s[3] += term(v[3], cb[u][1]);
                }
            }
            for (; c0 + kPerThread <= n_cols; c0 += kChunk) {
                double v[kPerThread];
                widen<L>(load_quad<L>(S, stride, r, c0), v);
                const v2f64* p = reinterpret_cast<const v2f64*>(cover + c0);
                const v2f64 ca = p[0], cb = p[1];
                s[0] += term(v[0], ca[0]), s[1] += term(v[1], ca[1]);
                s[2] += term(v[2], cb[0]), s[3] += term(v[3], cb[1]);
            }
        }
        for (; c0 < n_cols; c0 += kChunk) {                               // element by element: inside the block only
#pragma unroll
            for (int k = 0; k < kPerThread; ++k)
                if (c0 + k < n_cols) s[k] += term(elem<L>(S, stride, r, c0 + k), cover[c0 + k]);
        }
        double x = (s[0] + s[1]) + (s[2] + s[3]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
        if (lane == 0) s_wave[wave] = x;
        __syncthreads();
        if (tid == 0) gain[i] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        __syncthreads();                                                  // (the next listed row writes s_wave again)
    }
}

template <int L>
__global__ __launch_bounds__(kThreads) void cover_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                         int64_t n_cols, const int32_t* __restrict__ rows, int64_t n_list,
                                                         double* __restrict__ cover, unsigned* __restrict__ raised) {
    const int lane = threadIdx.x & 63;
    for (int64_t c0 = blockIdx.x * int64_t(kThreads); c0 < n_cols; c0 += int64_t(gridDim.x) * kThreads) {
        const int64_t c = c0 + threadIdx.x;
        const bool live = c < n_cols;
        double cov = live ? cover[c] : 0.0;
        for (int64_t i = 0; i < n_list; ++i) {
            const int64_t r = rows[i];
            if (r < 0 || r >= n_rows) continue;                           // (uniform over the workgroup)
            const double v = live ? elem<L>(S, stride, r, c) : 0.0;
            const bool up = live && v > cov;
            cov = up ? v : cov;
            const unsigned long long m = __ballot(up);
            if (lane == 0 && m) atomicAdd(raised + i, (unsigned)__popcll(m));
        }
        if (live) cover[c] = cov;
    }
}

int check_call(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols, int64_t n_list,
               const double* cover) {
    const int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    const uintptr_t p = reinterpret_cast<uintptr_t>(S);
    const unsigned size = layout == ROWMAJOR_F64 ? 8 : layout == PANEL_F16 ? 2 : 4;
    REQUIRE(p % size == 0, "S must start on a multiple of its element's size (%u bytes)", size);
    REQUIRE(n_list >= 0 && n_list < (int64_t(1) << 31), "bad number of listed rows %lld", (long long)n_list);
    REQUIRE(cover || n_cols == 0, "cover is NULL");
    REQUIRE(reinterpret_cast<uintptr_t>(cover) % 8 == 0, "cover must start on a multiple of 8 bytes");
    return 0;
}

}  // namespace

extern "C" {

int simrank_exemplars_version(void) { return SIMRANK_EXEMPLARS_VERSION; }

const char* simrank_exemplars_last_error(void) { return g_error.c_str(); }

int simrank_exemplars_gains(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                            const int32_t* rows, int64_t n_list, const double* cover, double* gain, void* stream) {
    const int rc = check_call(S, layout, stride, n_rows, n_cols, n_list, cover);
    if (rc) return rc;
    REQUIRE(rows || n_list == n_rows, "without rows, n_list (%lld) must be n_rows (%lld)", (long long)n_list,
            (long long)n_rows);
    REQUIRE(gain || n_list == 0, "gain is NULL");
    if (n_list == 0) return SIMRANK_EXEMPLARS_OK;
    const bool vec = n_rows > 0 && n_cols > 0 && quad_vector_loads(S, layout, stride) &&
                     reinterpret_cast<uintptr_t>(cover) % 16 == 0;
    const dim3 grid((unsigned)std::min<int64_t>(n_list, kGridCap));
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        if (vec)
            hipLaunchKernelGGL((gains_kernel<L, true>), grid, dim3(kThreads), 0, st, S, stride, n_rows, n_cols, rows,
                               n_list, cover, gain);
        else
            hipLaunchKernelGGL((gains_kernel<L, false>), grid, dim3(kThreads), 0, st, S, stride, n_rows, n_cols, rows,
                               n_list, cover, gain);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_EXEMPLARS_OK;
}

int simrank_exemplars_cover(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                            const int32_t* rows, int64_t n_list, double* cover, uint32_t* raised, void* stream) {
    const int rc = check_call(S, layout, stride, n_rows, n_cols, n_list, cover);
    if (rc) return rc;
    REQUIRE(n_list >= 1, "n_list must be at least 1 (got %lld)", (long long)n_list);
    REQUIRE(rows && raised, "rows or raised is NULL");
    if (n_cols == 0) return SIMRANK_EXEMPLARS_OK;
    const dim3 grid((unsigned)std::min<int64_t>((n_cols + kThreads - 1) / kThreads, kGridCap));
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL((cover_kernel<L>), grid, dim3(kThreads), 0, st, S, stride, n_rows, n_cols, rows, n_list, cover,
                           raised);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_EXEMPLARS_OK;
}

}  // extern "C"
