// What the companion libraries share, and nothing of the main library.  All twenty-one (select, f64, query, foldin, model, sets,
// neighbors, profile, cluster, rank, linkage, groups, kmedoids, explain, compare, diverse, operator, density, hdbscan, candidates, exemplars) take the error plumbing of a C entry point; all but f64 and rank (which reads a
// float64 score band, not an iterate) take the layouts a block of an iterate is read in, and what depends on them:
//     one element      Stored<L>, offset_of<L>, load<L>, elem<L>: query, sets, neighbors, model, groups, kmedoids, explain,
//                      compare, diverse, operator, density, hdbscan, candidates, exemplars
//     host checks      check_block: query, sets, neighbors, model, groups, kmedoids, explain, compare, diverse, operator, candidates, exemplars;
//                      plan_launch: select, profile, cluster, linkage, density, hdbscan;  quad_vector_loads: sets, kmedoids, compare, diverse, operator, exemplars
//     layout dispatch  with_layout, a runtime layout code as a template argument: all but model's pair dispatch
//     the 16-byte walk Elem<L>, WALK_GEOMETRY and WALK_LOAD, the lane geometry and the load phase of a sweep: select,
//                      profile, cluster, linkage, density, hdbscan
// Private and header-only: every name is in the anonymous namespace, so each library keeps its own message and exports
// nothing new.  A file names its library's two return codes before the include:
//     #define COMPANION_ERR_INVALID SIMRANK_QUERY_ERR_INVALID
//     #define COMPANION_ERR_HIP SIMRANK_QUERY_ERR_HIP
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <type_traits>

#if !defined(COMPANION_ERR_INVALID) || !defined(COMPANION_ERR_HIP)
#error "define COMPANION_ERR_INVALID and COMPANION_ERR_HIP before including companion.h"
#endif

namespace {

thread_local std::string g_error;          // what the library's *_last_error() returns

void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}

#define REQUIRE(cond, ...)                \
    do {                                  \
        if (!(cond)) {                    \
            set_error(__VA_ARGS__);       \
            return COMPANION_ERR_INVALID; \
        }                                 \
    } while (0)

#define HIP_CHECK(call)                                               \
    do {                                                              \
        hipError_t e_ = (call);                                       \
        if (e_ != hipSuccess) {                                       \
            set_error("%s failed: %s", #call, hipGetErrorString(e_)); \
            (void)hipGetLastError();                                  \
            return COMPANION_ERR_HIP;                                 \
        }                                                             \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---- layouts ---------------------------------------------------------------------------------------------------------------
// The layouts of a block of an iterate ("iterate_layout" of simrank_plan_get & co).  The public headers declare them
// under their own prefix; each library asserts that they are these.
enum Layout : int { PANEL_F32 = 0, ROWMAJOR_F32 = 1, PANEL_F16 = 2, ROWMAJOR_F64 = 3 };

#define COMPANION_SAME_LAYOUT(PREFIX, NAME) \
    static_assert(int(PREFIX##NAME) == NAME, "the public header's " #PREFIX #NAME " is not the shared layout code")

inline bool known_layout(int32_t layout) { return layout >= PANEL_F32 && layout <= ROWMAJOR_F64; }
inline bool is_panel(int32_t layout) { return layout == PANEL_F32 || layout == PANEL_F16; }

// f(std::integral_constant<int, layout>) for a runtime layout code: inside `[&](auto L) { ... }`, L is a template
// argument.  The caller has checked the code before (known_layout, check_block or plan_launch): an unknown one would
// run as ROWMAJOR_F64.  A library that serves fewer layouts discards the others with `if constexpr`.
template <class F>
inline void with_layout(int32_t layout, F&& f) {
    switch (layout) {
        case PANEL_F32: f(std::integral_constant<int, PANEL_F32>{}); break;
        case ROWMAJOR_F32: f(std::integral_constant<int, ROWMAJOR_F32>{}); break;
        case PANEL_F16: f(std::integral_constant<int, PANEL_F16>{}); break;
        default: f(std::integral_constant<int, ROWMAJOR_F64>{}); break;
    }
}

// ---- one element -----------------------------------------------------------------------------------------------------------
constexpr float kHalfScale = 1.0f / 16384.0f;          // fp16-held values are value x 2^14

template <int L> struct Stored { using type = float; };
template <> struct Stored<PANEL_F16> { using type = __half; };
template <> struct Stored<ROWMAJOR_F64> { using type = double; };

// element offset of (r, c) in layout L
template <int L>
__device__ inline int64_t offset_of(int64_t stride, int64_t r, int64_t c) {
    if constexpr (L == PANEL_F32) {
        return ((c >> 5) * stride + r) * 32 + (c & 31);
    } else if constexpr (L == PANEL_F16) {
        return ((c >> 6) * stride + r) * 64 + (c & 63);
    } else {
        return r * stride + c;
    }
}

// element (r, c) of a block in layout L as the dense hand-back widens it: a float, or the double of a float64 block
template <int L>
__device__ inline auto load(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c) {
    const auto x = static_cast<const typename Stored<L>::type*>(S)[offset_of<L>(stride, r, c)];
    if constexpr (L == PANEL_F16) return __half2float(x) * kHalfScale;
    else return x;
}

template <int L>
__device__ inline double elem(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c) {
    return (double)load<L>(S, stride, r, c);
}

// What every entry point that reads a block element by element refuses.  `what` names the block in the message.
inline int check_block(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                       const char* what = "S") {
    REQUIRE(known_layout(layout), "%s: unknown layout %d", what, (int)layout);
    REQUIRE(n_rows >= 0 && n_cols >= 0 && n_rows < (int64_t(1) << 31) && n_cols < (int64_t(1) << 31),
            "%s: bad block shape %lld x %lld", what, (long long)n_rows, (long long)n_cols);
    REQUIRE(S || n_rows == 0 || n_cols == 0, "%s is NULL", what);
    const bool panels = is_panel(layout);
    REQUIRE(stride >= (panels ? n_rows : n_cols), "%s: stride %lld is smaller than the block's %s (%lld)", what,
            (long long)stride, panels ? "rows" : "columns", (long long)(panels ? n_rows : n_cols));
    return 0;
}

// Whether every quad of 4 consecutive columns c .. c + 3 (c a multiple of 4) inside the block is one aligned vector load
// of 16 (f32), 8 (binary16) or 32 (float64) bytes: panels when the block starts on 16 (8) bytes (32 and 64 divide by 4, a
// panel row is 128 bytes); a row-major block when its rows start on 16 bytes.  sets, kmedoids, compare.
inline bool quad_vector_loads(const void* S, int32_t layout, int64_t stride) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(S);
    switch (layout) {
        case PANEL_F32: return p % 16 == 0;
        case PANEL_F16: return p % 8 == 0;
        case ROWMAJOR_F32: return p % 16 == 0 && stride % 4 == 0;
        default: return p % 16 == 0 && stride % 2 == 0;
    }
}

// ---- the 16-byte walk of a block -------------------------------------------------------------------------------------------
typedef unsigned v4u32 __attribute__((ext_vector_type(4)));

// What a 16-byte piece holds in each layout, and how a value widens.
template <int LAYOUT>
struct Elem {
    static constexpr bool ROWMAJOR = LAYOUT == ROWMAJOR_F32 || LAYOUT == ROWMAJOR_F64;
    static constexpr int V = LAYOUT == PANEL_F16 ? 8 : LAYOUT == ROWMAJOR_F64 ? 2 : 4;   // values per 16-byte load
    static constexpr int L = ROWMAJOR ? 64 : 8;                                          // lanes per row
    using Raw = typename std::conditional<LAYOUT == ROWMAJOR_F64, uint64_t, uint32_t>::type;     // the stored bits
    using Cmp = typename std::conditional<LAYOUT == ROWMAJOR_F64, double, float>::type;          // compared as

    __device__ static Raw raw(const v4u32& x, int i) {
        if constexpr (LAYOUT == ROWMAJOR_F64) return (uint64_t(x[2 * i + 1]) << 32) | x[2 * i];
        else if constexpr (LAYOUT == PANEL_F16) return (x[i >> 1] >> (16 * (i & 1))) & 0xffffu;
        else return x[i];
    }
    // the value as the dense hand-back widens it (fp16 -> f32 is exact, x 2^-14 is exact)
    __device__ static Cmp value(Raw b) {
        if constexpr (LAYOUT == ROWMAJOR_F64) return __longlong_as_double((long long)b);
        else if constexpr (LAYOUT == PANEL_F16) return float(__builtin_bit_cast(_Float16, (unsigned short)b)) * kHalfScale;
        else return __uint_as_float(b);
    }
};

// The row -> wave map of a sweep and its load phase.  Panel layouts: a wave takes EIGHT consecutive rows, lane group
// g = lane >> 3 owns row 8 w + g, lane q = lane & 7 the 16 bytes at 16 q of every panel's row segment, so one load
// instruction reads the eight rows' segments of a panel, 1 KiB contiguous.  Row-major: a wave takes one row, 16 bytes
// per lane, 1 KiB per load instruction.  A kernel walks `for (r0 = wave * R; r0 < n_rows; r0 += nwaves * R)` with its
// row r = r0 + g and, per row, `for (k0 = 0; k0 < n_chunks; k0 += U)` with one WALK_LOAD per turn; lane q's values of
// chunk k are the columns k * W + q * V onwards.
// WALK_GEOMETRY declares, in the scope it is used in, the constants V, L, R, W, U and the variables lane, g, q, wave,
// nwaves, n_chunks: a kernel that uses it may declare none of these names itself.  WALK_LOAD declares `x` (the name it
// is given) and needs U, V, W, q and n_chunks of WALK_GEOMETRY in scope; `u`, `k`, `i`, `c0`, `row` and `D` are local
// to it.  Both are macros that expand in the kernel's own scope, not functions: as functions they changed the instructions of
// every kernel that uses them (the workgroup's size is only a constant where the kernel itself reads it, and the loads
// were scheduled differently); profiles/companion_walk_ab.md has the comparison.
#define WALK_GEOMETRY(LAYOUT, n_cols)                                                                                 \
    constexpr int V = Elem<LAYOUT>::V, L = Elem<LAYOUT>::L;                                                           \
    constexpr int R = 64 / L; /* rows per wave */                                                                     \
    constexpr int W = L * V;  /* columns per chunk: a panel, or 64 x V columns of a row */                            \
    constexpr int U = 4;      /* chunks in flight */                                                                  \
    const int lane = threadIdx.x & 63, g = lane / L, q = lane % L;                                                    \
    const int64_t wave = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;                                       \
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;                                                    \
    const int64_t n_chunks = (n_cols + W - 1) / W

// v4u32 x[U]: x[u] = this lane's 16 bytes of chunk k0 + u of row r, zeros where the row is not live or the chunk or the
// columns are past the end: non-temporal vector loads, and a scalar tail where a row-major row ends or `vec`
// (plan_launch) is 0
#define WALK_LOAD(LAYOUT, x, S, stride, r, live, k0, n_cols, vec)                                                     \
    v4u32 x[U];                                                                                                       \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                                                                   \
        const int64_t k = k0 + u;                                                                                     \
        x[u] = v4u32{0, 0, 0, 0};                                                                                     \
        if (!live || k >= n_chunks) continue;                                                                         \
        if constexpr (!Elem<LAYOUT>::ROWMAJOR) {                                                                      \
            x[u] = __builtin_nontemporal_load(reinterpret_cast<const v4u32*>(S) + ((k * stride + r) * 8 + q));        \
        } else {                                                                                                      \
            constexpr int D = 4 / V; /* dwords per value */                                                           \
            const unsigned* row = reinterpret_cast<const unsigned*>(S) + r * stride * D;                              \
            const int64_t c0 = k * W + int64_t(V) * q;                                                                \
            if (vec && c0 + V - 1 < n_cols) {                                                                         \
                x[u] = __builtin_nontemporal_load(reinterpret_cast<const v4u32*>(row + c0 * D));                      \
            } else {                                                                                                  \
                _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                         \
                    if (c0 + i / D < n_cols) x[u][i] = row[c0 * D + i];                                               \
            }                                                                                                         \
        }                                                                                                             \
    }

// Host side of a sweep: what a swept block must be, and its launch: kSweepThreads per workgroup, whose four waves take
// consecutive rows (or groups of eight), at most kSweepMaxGrid workgroups.  `aligned_elements`: also refuse a row-major
// block that does not start on a multiple of its element's size (select never has).
constexpr int kSweepThreads = 256;
constexpr int kSweepMaxGrid = 256 * 8;

struct Launch {
    int grid, vec;
    int64_t rows;                                // the most rows one workgroup walks
};

inline int plan_launch(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols, bool aligned_elements,
                       Launch* out) {
    REQUIRE(known_layout(layout), "unknown layout %d", (int)layout);
    REQUIRE(n_rows >= 0 && n_cols >= 0 && n_cols < (int64_t(1) << 31) && n_rows < (int64_t(1) << 31),
            "bad block shape %lld x %lld", (long long)n_rows, (long long)n_cols);
    REQUIRE(n_rows == 0 || n_cols == 0 || S, "S is NULL");
    const bool rowmajor = !is_panel(layout);
    REQUIRE(rowmajor ? stride >= n_cols : stride >= n_rows, "stride %lld is too small for %lld x %lld", (long long)stride,
            (long long)n_rows, (long long)n_cols);
    const bool aligned = (reinterpret_cast<uintptr_t>(S) & 15) == 0;
    REQUIRE(rowmajor || aligned, "a panel-blocked block must be 16-byte aligned");
    if (aligned_elements) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(S);
        REQUIRE(layout != ROWMAJOR_F64 || (p & 7) == 0, "a float64 block must be 8-byte aligned");
        REQUIRE(layout != ROWMAJOR_F32 || (p & 3) == 0, "an f32 block must be 4-byte aligned");
    }
    const int64_t rows_per_wave = rowmajor ? 1 : 8;
    const int64_t waves = std::max<int64_t>(1, (n_rows + rows_per_wave - 1) / rows_per_wave);
    const int64_t per_group = kSweepThreads / 64;
    out->grid = (int)std::max<int64_t>(1, std::min<int64_t>((waves + per_group - 1) / per_group, kSweepMaxGrid));
    out->vec = rowmajor && aligned && (stride % (layout == ROWMAJOR_F64 ? 2 : 4)) == 0;
    const int64_t turns = (waves + out->grid * per_group - 1) / (out->grid * per_group);
    out->rows = turns * per_group * rows_per_wave;
    return 0;
}

}  // namespace
