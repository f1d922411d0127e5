// Diversified selection on the score band of the basket queries (include/simrank_diverse.h, libsimrank_diverse.so):
// greedy maximal-marginal-relevance picks, the penalty of a candidate the largest similarity any earlier pick's ROW
// holds for it, read IN PLACE from a block of the iterate in the layout its plan stores it, or from the neighbour
// tables of a pruned model.
//
//     pick    one workgroup per basket, at most k sweeps of its n_out candidates.  Sweep t does three things in one pass:
//             it applies the row of pick t - 1 to pen (skipped at t = 0, which writes the first pen vector instead), forms
//             value = (rel_w * score) - (lam * pen) with both products and the difference rounded separately, and reduces
//             the best candidate: within the lane, across the wave, across the workgroup, on a 64-bit order-preserving
//             integer key of the value (-0.0 canonicalised for the comparison only), then the smaller candidate: the
//             total order sets_topk and the neighbour selection use.  The lane that owns the winner still holds its
//             score, pen and value and writes them out with their own bits.  A picked or excluded candidate is marked
//             by a NaN in its pen (a pen is never NaN otherwise): its value is NaN and is never picked again, and no
//             x > NaN moves it.  A pen is +0.0, that mark or a stored element, so for f32 and binary16 blocks the workspace
//             holds it as f32, exactly, at half the bytes.  A lane owns four consecutive candidates per turn; without a
//             column map their scores, pens and row elements are 16-byte loads (8 of binary16, 2 x 16 of float64)
//             where block, band and workspace are aligned for them, and a pen quad is stored only when one of its
//             four changed.
//     lists   the same kernel: a row of P is +0.0 but for its list, so the row step is a scatter of the previous pick's kk
//             entries before the sweep (the ids of a row are distinct: no two lanes meet on one pen).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "simrank_diverse.h"

#define COMPANION_ERR_INVALID SIMRANK_DIVERSE_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_DIVERSE_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_DIVERSE_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_DIVERSE_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_DIVERSE_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_DIVERSE_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = 4;                              // candidates of one lane per turn
constexpr int kChunk = kThreads * kPerThread;              // candidates of one workgroup per turn
static_assert(kChunk == SIMRANK_DIVERSE_CHUNK, "the header's chunk is the kernel's");

// (rel_w * score) - (lam * pen) with three roundings: the compiler may not contract them into fused multiply-adds
__device__ __forceinline__ double value_of(double rel_w, double score, double lam, double pen) {
#pragma clang fp contract(off)
    const double a = rel_w * score;
    const double b = lam * pen;
    return a - b;
}

// an integer that orders as the double does (no NaN comes here); -0.0 and +0.0 get the same key
__device__ __forceinline__ uint64_t order_key(double v) {
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the best candidate so far: j < 0 = none yet
struct Best {
    uint64_t key;
    int32_t j;
};

__device__ __forceinline__ bool better(uint64_t key, int32_t j, const Best& than) {
    return j >= 0 && (than.j < 0 || key > than.key || (key == than.key && j < than.j));
}

// elements c .. c + 3 (c a multiple of 4, all four inside the block) of row r, widened; the 16 / 8 / 32 bytes are contiguous
template <int L>
__device__ __forceinline__ void load_quad(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c, double (&v)[4]) {
    if constexpr (L == PANEL_F32 || L == ROWMAJOR_F32) {
        const float4 x = *reinterpret_cast<const float4*>(static_cast<const float*>(S) + offset_of<L>(stride, r, c));
        v[0] = (double)x.x, v[1] = (double)x.y, v[2] = (double)x.z, v[3] = (double)x.w;
    } else if constexpr (L == PANEL_F16) {
        union {
            uint2 bits;
            __half h[4];
        } x;
        x.bits = *reinterpret_cast<const uint2*>(static_cast<const __half*>(S) + offset_of<L>(stride, r, c));
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) v[i] = (double)(__half2float(x.h[i]) * kHalfScale);
    } else {
        const double2* p = reinterpret_cast<const double2*>(static_cast<const double*>(S) + offset_of<L>(stride, r, c));
        const double2 a = p[0], b = p[1];
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    }
}

// four values at p[0 .. 3], widened, with 16-byte accesses (p on 16 bytes): two for doubles, one for floats
__device__ __forceinline__ void load4(const double* __restrict__ p, double (&v)[4]) {
    const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1];
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
}

__device__ __forceinline__ void load4(const float* __restrict__ p, double (&v)[4]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = (double)a.x, v[1] = (double)a.y, v[2] = (double)a.z, v[3] = (double)a.w;
}

__device__ __forceinline__ void store4(double* __restrict__ p, const double (&v)[4]) {
    reinterpret_cast<double2*>(p)[0] = double2{v[0], v[1]};
    reinterpret_cast<double2*>(p)[1] = double2{v[2], v[3]};
}

__device__ __forceinline__ void store4(float* __restrict__ p, const double (&v)[4]) {
    *reinterpret_cast<float4*>(p) = float4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// What a pen is held as in the workspace.  A pen is +0.0, a NaN mark or a stored element: where the elements are f32 or
// binary16 x 2^-14 it is exact in f32, which halves the bytes a sweep moves for it.  float64 blocks and the neighbour
// tables (doubles) keep doubles.
template <int L> struct PenOf { using type = float; };
template <> struct PenOf<ROWMAJOR_F64> { using type = double; };     // (the lists form is instantiated with this layout)

// The matrix a pick's row is read from.  LISTS: the tables of a pruned model (S, stride, n_rows, n_cols, row_pos and
// col_pos are not used); otherwise a block in layout L.  VEC: no column map and every quad inside the block is one
// aligned vector load.
struct Source {
    const void* S;
    int64_t stride, n_rows, n_cols;
    const int32_t* row_pos;
    const int32_t* col_pos;
    const int32_t* nbr_ids;
    const double* nbr_vals;
    int32_t kk;
};

// wide: the band's rows and the pen vectors are on 16 bytes
template <int L, bool VEC, bool LISTS>
__global__ __launch_bounds__(kThreads) void diverse_pick_kernel(Source src, int64_t n_out, const double* __restrict__ band,
                                                                int64_t ld_band, int64_t ld_pen, int k, double rel_w,
                                                                double lam, int wide, int32_t* __restrict__ idx_out,
                                                                double* __restrict__ score_out,
                                                                double* __restrict__ pen_out,
                                                                double* __restrict__ val_out, double* __restrict__ pens) {
    __shared__ uint64_t s_key[kWaves];
    __shared__ int32_t s_j[kWaves];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* __restrict__ row = band + q * ld_band;
    using Pen = typename PenOf<L>::type;
    Pen* __restrict__ pen = reinterpret_cast<Pen*>(pens + q * ld_pen);    // (every vector starts where a double one would)
    const double nan = __builtin_nan(""), ninf = -__builtin_inf();
    int32_t* idx = idx_out + q * int64_t(k);
    double *so = score_out + q * int64_t(k), *po = pen_out + q * int64_t(k), *vo = val_out + q * int64_t(k);

    int32_t prev = -1;                                     // the previous pick
    int t = 0;
    for (; t < k; ++t) {
        // the previous pick's row: a block row, or its list scattered into pen before the sweep
        int64_t r = -1;
        bool row_ok = false;
        if (t > 0) {
            if constexpr (LISTS) {
                const int32_t* ids = src.nbr_ids + int64_t(prev) * src.kk;
                const double* vals = src.nbr_vals + int64_t(prev) * src.kk;
                for (int e = tid; e < src.kk; e += kThreads) {
                    const int64_t b = ids[e];
                    if (b >= 0 && b < n_out) {
                        const double x = vals[e];
                        if (x > (double)pen[b]) pen[b] = (Pen)x;        // (a NaN pen, a picked or excluded candidate, stays)
                    }
                }
                __syncthreads();
            } else {
                r = src.row_pos ? int64_t(src.row_pos[prev]) : int64_t(prev);
                row_ok = r >= 0 && r < src.n_rows;
            }
        }
        Best best{0, -1};
        double b_score = 0.0, b_pen = 0.0, b_value = 0.0;
        for (int64_t j0 = int64_t(tid) * kPerThread; j0 < n_out; j0 += kChunk) {
            const bool full = j0 + kPerThread <= n_out;
            double s[kPerThread], p[kPerThread];
            if (wide && full) {
                load4(row + j0, s);
            } else {
#pragma unroll
                for (int i = 0; i < kPerThread; ++i) s[i] = j0 + i < n_out ? row[j0 + i] : nan;
            }
            bool changed = false;
            if (t == 0) {
#pragma unroll
                for (int i = 0; i < kPerThread; ++i) p[i] = s[i] > ninf ? 0.0 : nan;      // (s > -inf: false for NaN too)
                changed = true;
            } else {
                if (wide && full) {
                    load4(pen + j0, p);
                } else {
#pragma unroll
                    for (int i = 0; i < kPerThread; ++i) p[i] = j0 + i < n_out ? (double)pen[j0 + i] : nan;
                }
                if constexpr (!LISTS) {
                    double x[kPerThread];
                    if (!row_ok) {
#pragma unroll
                        for (int i = 0; i < kPerThread; ++i) x[i] = nan;
                    } else if (VEC && full && j0 + kPerThread <= src.n_cols) {
                        load_quad<L>(src.S, src.stride, r, j0, x);
                    } else {
#pragma unroll
                        for (int i = 0; i < kPerThread; ++i) {
                            x[i] = nan;
                            if (j0 + i < n_out) {
                                const int64_t c = src.col_pos ? int64_t(src.col_pos[j0 + i]) : j0 + i;
                                if (c >= 0 && c < src.n_cols) x[i] = elem<L>(src.S, src.stride, r, c);
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < kPerThread; ++i)
                        if (x[i] > p[i]) p[i] = x[i], changed = true;
                }
#pragma unroll
                for (int i = 0; i < kPerThread; ++i)
                    if (j0 + i == prev) p[i] = nan, changed = true;
            }
            if (changed) {
                if (wide && full) {
                    store4(pen + j0, p);
                } else {
#pragma unroll
                    for (int i = 0; i < kPerThread; ++i)
                        if (j0 + i < n_out) pen[j0 + i] = (Pen)p[i];
                }
            }
#pragma unroll
            for (int i = 0; i < kPerThread; ++i) {
                const double v = value_of(rel_w, s[i], lam, p[i]);
                if (v == v) {                              // (NaN: a dead candidate, a NaN score, or 0 x inf)
                    const uint64_t key = order_key(v);
                    const int32_t j = int32_t(j0 + i);
                    if (better(key, j, best)) best = Best{key, j}, b_score = s[i], b_pen = p[i], b_value = v;
                }
            }
        }
        // the workgroup's best: across the wave, then across the waves
        Best all = best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t ok = __shfl_xor(all.key, off);
            const int32_t oj = __shfl_xor(all.j, off);
            if (better(ok, oj, all)) all = Best{ok, oj};
        }
        if (lane == 0) s_key[wave] = all.key, s_j[wave] = all.j;
        __syncthreads();
        all = Best{s_key[0], s_j[0]};
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            if (better(s_key[w], s_j[w], all)) all = Best{s_key[w], s_j[w]};
        __syncthreads();                                   // (s_key and s_j are written again in the next sweep)
        if (all.j < 0) break;
        if (best.j == all.j) {                             // the one lane that owns the winner
            idx[t] = all.j;
            so[t] = b_score, po[t] = b_pen, vo[t] = b_value;
        }
        prev = all.j;
    }
    for (int tt = t + tid; tt < k; tt += kThreads) {
        idx[tt] = -1;
        so[tt] = 0.0, po[tt] = 0.0, vo[tt] = 0.0;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
bool sizes_ok(int64_t n_sets, int64_t n_out) {
    return n_sets >= 0 && n_out >= 0 && n_sets < (int64_t(1) << 31) && n_out < (int64_t(1) << 31);
}

int64_t pen_stride(int64_t n_out) { return (n_out + 1) & ~int64_t(1); }       // doubles: every pen vector on 16 bytes

int check_common(int64_t n_out, const double* band, int64_t ld_band, int64_t n_sets, int32_t k, double rel_w, double lam,
                 const int32_t* idx_out, const double* score_out, const double* pen_out, const double* val_out,
                 const void* workspace) {
    REQUIRE(sizes_ok(n_sets, n_out) && ld_band >= n_out, "bad band shape %lld x %lld (ld %lld)", (long long)n_sets,
            (long long)n_out, (long long)ld_band);
    REQUIRE(k >= 1, "k must be positive (got %d)", (int)k);
    REQUIRE(int64_t(k) * n_sets < (int64_t(1) << 40), "k x baskets is too large");
    REQUIRE(std::isfinite(rel_w) && lam >= 0.0 && lam <= 1.0, "rel_w must be finite and lam in [0, 1] (got %g, %g)", rel_w,
            lam);
    REQUIRE(n_sets <= SIMRANK_DIVERSE_MAX_BLOCKS, "%lld baskets are too many for one call: cut them into bands",
            (long long)n_sets);
    if (n_sets == 0) return 0;
    REQUIRE(idx_out && score_out && pen_out && val_out, "an output is NULL");
    REQUIRE((band && workspace) || n_out == 0, "band or workspace is NULL");
    REQUIRE(reinterpret_cast<uintptr_t>(band) % 8 == 0 && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
            "band and workspace must be 8-byte aligned");
    return 0;
}

bool wide_rows(const double* band, int64_t ld_band, const void* workspace) {
    return reinterpret_cast<uintptr_t>(band) % 16 == 0 && ld_band % 2 == 0 && reinterpret_cast<uintptr_t>(workspace) % 16 == 0;
}

}  // namespace

extern "C" {

int simrank_diverse_version(void) { return SIMRANK_DIVERSE_VERSION; }

const char* simrank_diverse_last_error(void) { return g_error.c_str(); }

int64_t simrank_diverse_blocks(int64_t n_sets, int64_t n_out) { return sizes_ok(n_sets, n_out) ? n_sets : -1; }

int64_t simrank_diverse_workspace_bytes(int64_t n_sets, int64_t n_out) {
    return sizes_ok(n_sets, n_out) ? n_sets * pen_stride(n_out) * 8 : -1;
}

int simrank_diverse_pick(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                         const int32_t* row_pos, const int32_t* col_pos, int64_t n_out, const double* band, int64_t ld_band,
                         int64_t n_sets, int32_t k, double rel_w, double lam, int32_t* idx_out, double* score_out,
                         double* pen_out, double* val_out, void* workspace, void* stream) {
    int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    rc = check_common(n_out, band, ld_band, n_sets, k, rel_w, lam, idx_out, score_out, pen_out, val_out, workspace);
    if (rc) return rc;
    if (n_sets == 0) return SIMRANK_DIVERSE_OK;
    const Source src{S, stride, n_rows, n_cols, row_pos, col_pos, nullptr, nullptr, 0};
    const bool vec = !col_pos && quad_vector_loads(S, layout, stride);
    const int wide = wide_rows(band, ld_band, workspace);
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)n_sets);
    with_layout(layout, [&](auto L) {
        if (vec)
            hipLaunchKernelGGL((diverse_pick_kernel<L, true, false>), grid, dim3(kThreads), 0, st, src, n_out, band, ld_band,
                               pen_stride(n_out), (int)k, rel_w, lam, wide, idx_out, score_out, pen_out, val_out,
                               static_cast<double*>(workspace));
        else
            hipLaunchKernelGGL((diverse_pick_kernel<L, false, false>), grid, dim3(kThreads), 0, st, src, n_out, band, ld_band,
                               pen_stride(n_out), (int)k, rel_w, lam, wide, idx_out, score_out, pen_out, val_out,
                               static_cast<double*>(workspace));
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_DIVERSE_OK;
}

int simrank_diverse_pick_lists(const int32_t* nbr_ids, const double* nbr_vals, const double* diag, int64_t n, int32_t kk,
                               const double* band, int64_t ld_band, int64_t n_sets, int32_t k, double rel_w, double lam,
                               int32_t* idx_out, double* score_out, double* pen_out, double* val_out, void* workspace,
                               void* stream) {
    (void)diag;                                            // (it meets only the pick's own pen: see the header)
    REQUIRE(kk >= 0, "kk must not be negative (got %d)", (int)kk);
    const int rc = check_common(n, band, ld_band, n_sets, k, rel_w, lam, idx_out, score_out, pen_out, val_out, workspace);
    if (rc) return rc;
    REQUIRE((nbr_ids && nbr_vals) || kk == 0 || n == 0, "nbr_ids or nbr_vals is NULL");
    if (n_sets == 0) return SIMRANK_DIVERSE_OK;
    const Source src{nullptr, 0, n, n, nullptr, nullptr, nbr_ids, nbr_vals, kk};
    hipLaunchKernelGGL((diverse_pick_kernel<ROWMAJOR_F64, false, true>), dim3((unsigned)n_sets), dim3(kThreads), 0,
                       as_stream(stream), src, n, band, ld_band, pen_stride(n), (int)k, rel_w, lam,
                       wide_rows(band, ld_band, workspace), idx_out, score_out, pen_out, val_out,
                       static_cast<double*>(workspace));
    HIP_CHECK(hipGetLastError());
    return SIMRANK_DIVERSE_OK;
}

}  // extern "C"
