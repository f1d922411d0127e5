// How far apart two iterates are, measured where they lie (include/simrank_compare.h, libsimrank_compare.so): one sweep of
// two blocks over the same rows and columns, each in its own layout, and per row the largest absolute and relative
// difference with their columns, the columns above each tolerance, and over the block a histogram of the differences'
// exponents.  Maxima and integer counts only: there is no floating-point sum in this file.
//
// The two layouts of a pair have different walk geometries, so this file does not use companion.h's 16-byte walk.  A
// wave takes one row; a lane owns the quad of four consecutive columns c .. c + 3 (c a multiple of 4) in BOTH blocks,
// one 16-, 8- or 32-byte load per side (a quad never crosses a panel: 32 and 64 divide by 4), as sets.hip and
// kmedoids.hip load; kInFlight quads per side are loaded before the first is consumed, 1024 columns of a row a turn.
// A side whose quads are not aligned vector loads (quad_vector_loads) is read element by element, as is the ragged last
// quad of a row-major row: no load leaves a block, and the padding columns of a panel are loaded but never counted.
//
// Where two models agree the difference is +0.0 (on a sparse iterate, almost everywhere).  A lane counts those in a register and only the elements
// that differ take the slow path (the tolerances, the division, the maxima, the bins), which the wave enters together
// when any lane has one.  The histogram lives in 8 KiB of local memory per workgroup as 32-bit bins: equal bins are
// aggregated across the wave first, as profile.hip's bump does, the rest add 1 per lane; the bins go to the caller's
// 64-bit counters once, at the workgroup's end.  The per-row results are reduced across the wave with shuffles in one
// total order (value descending, column ascending; the non-negative doubles compared as their bits) and stored by lane
// 0: no atomics for them.
#include "simrank_compare.h"

#define COMPANION_ERR_INVALID SIMRANK_COMPARE_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_COMPARE_ERR_HIP
#include "companion.h"

#include <cmath>

// d and rel are one subtraction and one division, each rounded once
#pragma clang fp contract(off)

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_COMPARE_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_COMPARE_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_COMPARE_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_COMPARE_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxTol = SIMRANK_COMPARE_MAX_TOL;
constexpr int kBins = SIMRANK_COMPARE_BINS;
constexpr int kMaxGrid = SIMRANK_COMPARE_MAX_GRID;
constexpr int kQuad = 4;                                   // columns of one lane's load
constexpr int kChunk = 64 * kQuad;                         // columns of one load instruction of a wave
constexpr int kInFlight = 4;                               // quads per side loaded before the first is consumed
constexpr int32_t kNoColumn = 0x7fffffff;
constexpr uint64_t kInfBits = 0x7ff0000000000000ull;

struct Tolerances {
    double t[kMaxTol];                                     // +inf past n_tol: nothing is above it
};

struct Quad {
    double v[kQuad];
};

typedef float v4f32 __attribute__((ext_vector_type(4)));
typedef double v2f64 __attribute__((ext_vector_type(2)));
typedef unsigned v2u32 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double widen_half(unsigned h) {
    return (double)(float(__builtin_bit_cast(_Float16, (unsigned short)h)) * kHalfScale);
}

// the quad at columns c .. c + 3 of row r as one aligned vector load, widened
template <int L>
__device__ __forceinline__ Quad load_quad(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c) {
    Quad q;
    const int64_t at = offset_of<L>(stride, r, c);
    if constexpr (L == PANEL_F32 || L == ROWMAJOR_F32) {
        const v4f32 x = __builtin_nontemporal_load(reinterpret_cast<const v4f32*>(static_cast<const float*>(S) + at));
#pragma unroll
        for (int i = 0; i < kQuad; ++i) q.v[i] = (double)x[i];
    } else if constexpr (L == PANEL_F16) {
        const v2u32 x = __builtin_nontemporal_load(reinterpret_cast<const v2u32*>(static_cast<const __half*>(S) + at));
#pragma unroll
        for (int i = 0; i < kQuad; ++i) q.v[i] = widen_half((x[i >> 1] >> (16 * (i & 1))) & 0xffffu);
    } else {
        const v2f64* p = reinterpret_cast<const v2f64*>(static_cast<const double*>(S) + at);
        const v2f64 lo = __builtin_nontemporal_load(p), hi = __builtin_nontemporal_load(p + 1);
        q.v[0] = lo[0], q.v[1] = lo[1], q.v[2] = hi[0], q.v[3] = hi[1];
    }
    return q;
}

// This lane's quad at column c of row r: zeros where the column is past n_cols.  `vec`: the side's quads are aligned
// vector loads.  A panel's row segment holds whole quads, padding included; a row-major row's last quad may be ragged.
template <int L>
__device__ __forceinline__ Quad fetch(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c, int64_t n_cols,
                                      int vec) {
    constexpr bool panel = L == PANEL_F32 || L == PANEL_F16;
    Quad q = {{0.0, 0.0, 0.0, 0.0}};
    if (c >= n_cols) return q;
    if (vec && (panel || c + kQuad <= n_cols)) return load_quad<L>(S, stride, r, c);
#pragma unroll
    for (int i = 0; i < kQuad; ++i)
        if (c + i < n_cols) q.v[i] = elem<L>(S, stride, r, c + i);
    return q;
}

// the bits of d(a, b): never NaN, never negative
__device__ __forceinline__ uint64_t distance_bits(double a, double b) {
    double d;
    if (a == b) {
        d = 0.0;
    } else {
        const bool na = a != a, nb = b != b;
        if (na || nb) d = (na && nb) ? 0.0 : __builtin_inf();
        else d = __builtin_fabs(a - b);
    }
    return (uint64_t)__double_as_longlong(d);
}

// (bits, column) comes before (best, best_c) in the order (value descending, column ascending)
__device__ __forceinline__ bool before(uint64_t bits, int32_t c, uint64_t best, int32_t best_c) {
    return bits > best || (bits == best && c < best_c);
}

__device__ __forceinline__ void wave_best(uint64_t& bits, int32_t& c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t ob = __shfl_xor((unsigned long long)bits, off);
        const int32_t oc = __shfl_xor(c, off);
        if (before(ob, oc, bits, c)) {
            bits = ob;
            c = oc;
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One element's bin into the workgroup's bins, called by every lane of the wave together (`in`: this lane has one):
// up to two rounds of (the first pending lane's bin, the lanes that share it, one add of their number), then singly.
__device__ __forceinline__ void bump(uint32_t* bins, bool in, uint32_t j, int lane) {
    uint64_t pending = __ballot(in);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (!pending) break;                                             // (wave-uniform)
        const int lead = __ffsll((unsigned long long)pending) - 1;
        const uint32_t j0 = (uint32_t)__builtin_amdgcn_readlane((int)j, lead);
        const uint64_t same = __ballot(in && j == j0);
        if (lane == lead) atomicAdd(&bins[j0], (uint32_t)__popcll(same));
        pending &= ~same;
        in = in && j != j0;
    }
    if (in) atomicAdd(&bins[j], 1u);
}

template <int LA, int LB>
__global__ __launch_bounds__(kThreads) void compare_kernel(const void* __restrict__ A, int64_t stride_a, int vec_a,
                                                           const void* __restrict__ B, int64_t stride_b, int vec_b,
                                                           int64_t n_rows, int64_t n_cols, Tolerances tol, int n_tol,
                                                           double floor, double* __restrict__ max_abs,
                                                           int32_t* __restrict__ arg_abs, double* __restrict__ max_rel,
                                                           int32_t* __restrict__ arg_rel, uint32_t* __restrict__ over,
                                                           unsigned long long* __restrict__ hist) {
    __shared__ uint32_t bins[kBins];
    for (int i = threadIdx.x; i < kBins; i += kThreads) bins[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * int64_t(kThreads) + threadIdx.x) >> 6;
    const int64_t nwaves = int64_t(gridDim.x) * kWaves;
    uint32_t zeros = 0;                                    // this lane's elements with d == +0.0, over all its rows

    for (int64_t r = wave; r < n_rows; r += nwaves) {
        uint64_t best_d = 0, best_rel = 0;                 // only elements that differ compete: all equal is (0.0, column 0)
        int32_t at_d = kNoColumn, at_rel = kNoColumn;
        uint32_t above[kMaxTol];
#pragma unroll
        for (int t = 0; t < kMaxTol; ++t) above[t] = 0;

        for (int64_t c0 = 0; c0 < n_cols; c0 += int64_t(kInFlight) * kChunk) {
            Quad a[kInFlight], b[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                const int64_t c = c0 + int64_t(u) * kChunk + lane * kQuad;
                a[u] = fetch<LA>(A, stride_a, r, c, n_cols, vec_a);
                b[u] = fetch<LB>(B, stride_b, r, c, n_cols, vec_b);
            }
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                const int64_t c = c0 + int64_t(u) * kChunk + lane * kQuad;
#pragma unroll
                for (int i = 0; i < kQuad; ++i) {
                    const bool in = c + i < n_cols;
                    const uint64_t d = distance_bits(a[u].v[i], b[u].v[i]);   // (both zero past n_cols: d == 0)
                    const bool differs = in && d != 0;
                    zeros += (in && d == 0) ? 1u : 0u;
                    if (!__ballot(differs)) continue;                    // (wave-uniform)
                    if (differs) {
                        const double dd = __longlong_as_double((long long)d);
#pragma unroll
                        for (int t = 0; t < kMaxTol; ++t) above[t] += dd > tol.t[t] ? 1u : 0u;
                        if (d > best_d) {                                // (a lane's columns ascend: the first of a tie stays)
                            best_d = d;
                            at_d = int32_t(c + i);
                        }
                        // the rules in the header's order: below the floor first (a NaN operand is below nothing), then
                        // d == inf (also where a finite difference overflowed), then the division
                        uint64_t rel = kInfBits;
                        if (a[u].v[i] == a[u].v[i] && b[u].v[i] == b[u].v[i]) {
                            const double m = __builtin_fmax(__builtin_fabs(a[u].v[i]), __builtin_fabs(b[u].v[i]));
                            if (m < floor) rel = 0;
                            else if (d != kInfBits) rel = (uint64_t)__double_as_longlong(dd / m);
                        }
                        if (rel > best_rel) {
                            best_rel = rel;
                            at_rel = int32_t(c + i);
                        }
                    }
                    bump(bins, differs, uint32_t(d >> 52), lane);
                }
            }
        }

        wave_best(best_d, at_d);
        wave_best(best_rel, at_rel);
#pragma unroll
        for (int t = 0; t < kMaxTol; ++t)
            if (t < n_tol) above[t] = wave_sum(above[t]);                // (n_tol is uniform)
        if (lane == 0) {
            const int32_t first = n_cols > 0 ? 0 : -1;                   // the smallest column attaining a maximum of 0.0
            max_abs[r] = __longlong_as_double((long long)best_d);
            arg_abs[r] = best_d ? at_d : first;
            max_rel[r] = __longlong_as_double((long long)best_rel);
            arg_rel[r] = best_rel ? at_rel : first;
#pragma unroll
            for (int t = 0; t < kMaxTol; ++t)
                if (t < n_tol) over[r * n_tol + t] = above[t];
        }
    }

    // bin 0: every lane's zeros, once per wave (the launch keeps a workgroup's elements below 2^32)
    zeros = wave_sum(zeros);
    if (lane == 0 && zeros) atomicAdd(&bins[0], zeros);
    __syncthreads();
    for (int b = threadIdx.x; b < kBins; b += kThreads)
        if (bins[b]) atomicAdd(&hist[b], (unsigned long long)bins[b]);
}

int check_aligned(const void* S, int32_t layout, const char* what) {
    const unsigned size = layout == ROWMAJOR_F64 ? 8 : layout == PANEL_F16 ? 2 : 4;
    REQUIRE(reinterpret_cast<uintptr_t>(S) % size == 0, "%s must start on a multiple of its element's size (%u bytes)", what,
            size);
    return 0;
}

}  // namespace

extern "C" {

int simrank_compare_version(void) { return SIMRANK_COMPARE_VERSION; }

const char* simrank_compare_last_error(void) { return g_error.c_str(); }

int simrank_compare_sweep(const void* A, int32_t layout_a, int64_t stride_a, const void* B, int32_t layout_b,
                          int64_t stride_b, int64_t n_rows, int64_t n_cols, const double* tol, int32_t n_tol, double floor,
                          double* max_abs, int32_t* arg_abs, double* max_rel, int32_t* arg_rel, uint32_t* over,
                          unsigned long long* hist, void* stream) {
    int rc = check_block(A, layout_a, stride_a, n_rows, n_cols, "A");
    if (rc) return rc;
    rc = check_block(B, layout_b, stride_b, n_rows, n_cols, "B");
    if (rc) return rc;
    rc = check_aligned(A, layout_a, "A");
    if (rc) return rc;
    rc = check_aligned(B, layout_b, "B");
    if (rc) return rc;
    REQUIRE(n_tol >= 0 && n_tol <= kMaxTol, "n_tol must be 0 .. %d (got %d)", kMaxTol, (int)n_tol);
    REQUIRE(tol || n_tol == 0, "tol is NULL");
    REQUIRE(!tol || n_tol > 0, "tol must be NULL when n_tol is 0");
    Tolerances ts;
    for (int t = 0; t < kMaxTol; ++t) ts.t[t] = INFINITY;
    for (int t = 0; t < n_tol; ++t) {
        REQUIRE(std::isfinite(tol[t]) && tol[t] >= 0.0, "tol[%d] = %g is not a finite number >= 0", t, tol[t]);
        ts.t[t] = tol[t];
    }
    REQUIRE(std::isfinite(floor) && floor >= 0.0, "floor = %g is not a finite number >= 0", floor);
    REQUIRE(n_rows == 0 || (max_abs && arg_abs && max_rel && arg_rel), "max_abs, arg_abs, max_rel or arg_rel is NULL");
    REQUIRE(over || n_tol == 0 || n_rows == 0, "over is NULL");
    REQUIRE(!over || n_tol > 0, "over must be NULL when n_tol is 0");
    REQUIRE(hist || n_rows == 0 || n_cols == 0, "hist is NULL");
    if (n_rows == 0) return SIMRANK_COMPARE_OK;
    const int64_t grid = std::min<int64_t>((n_rows + kWaves - 1) / kWaves, kMaxGrid);
    const int64_t turns = (n_rows + grid * kWaves - 1) / (grid * kWaves);
    REQUIRE((double)std::min<int64_t>(turns * kWaves, n_rows) * (double)n_cols < 4294967296.0,
            "a block of %lld x %lld gives one workgroup 2^32 elements or more: sweep it in bands of fewer rows",
            (long long)n_rows, (long long)n_cols);
    const int vec_a = quad_vector_loads(A, layout_a, stride_a), vec_b = quad_vector_loads(B, layout_b, stride_b);
    hipStream_t st = as_stream(stream);
    with_layout(layout_a, [&](auto LA) {
        with_layout(layout_b, [&](auto LB) {
            hipLaunchKernelGGL((compare_kernel<decltype(LA)::value, decltype(LB)::value>), dim3((unsigned)grid), dim3(kThreads), 0, st, A, stride_a, vec_a, B,
                               stride_b, vec_b, n_rows, n_cols, ts, (int)n_tol, floor, max_abs, arg_abs, max_rel, arg_rel,
                               over, hist);
        });
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_COMPARE_OK;
}

}  // extern "C"
