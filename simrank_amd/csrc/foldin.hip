// Fold-in on an iterate that stays on the device (include/simrank_foldin.h, libsimrank_foldin.so): the row the next
// update would compute for a node that was NOT in the fitted graph, from its neighbour list, with every existing
// similarity and normalisation held fixed.  One "leg 1" for a handful of rows and one "leg 2" against all of W with a
// skinny right-hand side, for tiles of up to 32 new nodes:
//
//     gather  T[id(c)][q] = w_q * sum_{i in I_q} S[pos(i)][c].  A workgroup owns 256 columns (128 in float64) of the
//             block and sums them for all 32 new nodes of the tile: each wave takes every fourth new node and walks its
//             list with one 16-byte load per lane and entry (8 bytes on binary16 panels), so a source row that several
//             new nodes share is fetched by ONE workgroup, from HBM once and from its XCD's L2 afterwards.  The sums go
//             through LDS to be written TRANSPOSED, whole 128-byte lines of T[n_src][32]: stage 2 then fetches one line
//             per neighbour for 32 new nodes, the access shape of the project's gather legs.
//     member  bit q of member[j] = j in I_q (integer atomic OR: order-free), the new half of the evidence count.
//     apply   acc[q] = sum_{j in I(b)} T[j][q], cnt[q] = sum_j member[j] bit q for every fitted node b.  Half a wave per
//             row (lane = new node: one line per entry, four entries in flight, four partial sums added in a fixed
//             order), two rows per wave, 32 rows per workgroup so that the float64 results leave through LDS as 256-byte
//             runs of out[q][b0 .. b0 + 31]; rows longer than SIMRANK_FOLDIN_LONG_ROW go to a second kernel, one
//             workgroup of 32 half waves per row, 32 strided partial sums added in a fixed order.  No floating-point atomics anywhere:
//             the same call gives the same bits twice.  The epilogue is float64 (scale, coefficient, evidence by ldexp,
//             prior blend).
#include <cstdio>
#include <string>

#include "simrank_foldin.h"

#define COMPANION_ERR_INVALID SIMRANK_FOLDIN_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_FOLDIN_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_FOLDIN_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_FOLDIN_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_FOLDIN_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_FOLDIN_, ROWMAJOR_F64);

constexpr int kTile = SIMRANK_FOLDIN_TILE;
constexpr int kLongRow = SIMRANK_FOLDIN_LONG_ROW;
static_assert(kTile == 32, "a tile is half a wave and one member word");

// what a lane of the gather reads per list entry, and the type the sums (and T) are kept in
template <int L>
struct Lay {
    using acc_t = float;
    static constexpr int kCols = 4;
};
template <>
struct Lay<SIMRANK_FOLDIN_ROWMAJOR_F64> {
    using acc_t = double;
    static constexpr int kCols = 2;
};

// acc[i] += element (r, c + i) of the block for i < kCols, widened as the dense hand-back widens it; one vector load when
// the run is inside the block (and, row-major, VEC says that rows start on 16 bytes)
template <int L, bool VEC>
__device__ inline void add_run(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c, int64_t n_cols,
                               typename Lay<L>::acc_t* acc) {
    constexpr int K = Lay<L>::kCols;
    const bool whole = c + K <= n_cols;
    if constexpr (L == SIMRANK_FOLDIN_PANEL_F32 || L == SIMRANK_FOLDIN_ROWMAJOR_F32) {
        const float* p = static_cast<const float*>(S) +
                         (L == SIMRANK_FOLDIN_PANEL_F32 ? ((c >> 5) * stride + r) * 32 + (c & 31) : r * stride + c);
        if (whole && (VEC || L == SIMRANK_FOLDIN_PANEL_F32)) {
            const float4 v = *reinterpret_cast<const float4*>(p);
            acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
        } else {
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (c + i < n_cols) acc[i] += p[i];
        }
    } else if constexpr (L == SIMRANK_FOLDIN_PANEL_F16) {
        const __half* p = static_cast<const __half*>(S) + ((c >> 6) * stride + r) * 64 + (c & 63);
        if (whole) {
            union { uint2 u; __half h[4]; } v;
            v.u = *reinterpret_cast<const uint2*>(p);
#pragma unroll
            for (int i = 0; i < K; ++i) acc[i] += __half2float(v.h[i]) * kHalfScale;
        } else {
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (c + i < n_cols) acc[i] += __half2float(p[i]) * kHalfScale;
        }
    } else {
        const double* p = static_cast<const double*>(S) + r * stride + c;
        if (whole && VEC) {
            const double2 v = *reinterpret_cast<const double2*>(p);
            acc[0] += v.x; acc[1] += v.y;
        } else {
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (c + i < n_cols) acc[i] += p[i];
        }
    }
}

template <int L, bool VEC>
__global__ __launch_bounds__(256) void foldin_gather_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                            int64_t n_cols, const int32_t* __restrict__ col_ids,
                                                            int64_t col_base, const int32_t* __restrict__ list_ptr,
                                                            const int32_t* __restrict__ list_pos,
                                                            const double* __restrict__ w, int n_tile,
                                                            typename Lay<L>::acc_t* __restrict__ T, int64_t n_src) {
    using A = typename Lay<L>::acc_t;
    constexpr int K = Lay<L>::kCols;
    constexpr int BC = 64 * K;                         // columns of one workgroup
    __shared__ A tile[BC][kTile + 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = int64_t(blockIdx.x) * BC + lane * K;
    for (int q = wave; q < kTile; q += 4) {
        A acc[K];
#pragma unroll
        for (int i = 0; i < K; ++i) acc[i] = A(0);
        if (q < n_tile) {
            const int lo = list_ptr[q], hi = list_ptr[q + 1];
            if (c < n_cols) {
#pragma unroll 4
                for (int e = lo; e < hi; ++e) {
                    const int64_t r = list_pos[e];
                    if (r >= 0 && r < n_rows) {
                        add_run<L, VEC>(S, stride, r, c, n_cols, acc);
                    } else {
#pragma unroll
                        for (int i = 0; i < K; ++i) acc[i] += A(__builtin_nanf(""));
                    }
                }
            }
            const double wq = w[q];
#pragma unroll
            for (int i = 0; i < K; ++i) acc[i] = A(wq * double(acc[i]));
        }
#pragma unroll
        for (int i = 0; i < K; ++i) tile[lane * K + i][q] = acc[i];
    }
    __syncthreads();
    // whole lines of T: four values (one 16- or 32-byte piece of a line) per thread and step, eight threads per line
    for (int idx = threadIdx.x; idx < BC * 8; idx += 256) {
        const int cl = idx >> 3, q4 = (idx & 7) * 4;
        const int64_t cc = int64_t(blockIdx.x) * BC + cl;
        if (cc >= n_cols) continue;
        const int64_t id = col_ids ? int64_t(col_ids[cc]) : col_base + cc;
        if (id < 0 || id >= n_src) continue;
        A* t = T + id * kTile + q4;
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = tile[cl][q4 + i];
    }
}

__global__ __launch_bounds__(256) void foldin_member_kernel(const int32_t* __restrict__ list_ptr,
                                                            const int32_t* __restrict__ list_ids,
                                                            const double* __restrict__ w, uint32_t* __restrict__ member,
                                                            int64_t n_src) {
    const int q = blockIdx.x;
    if (!(w[q] > 0.0)) return;                         // (a dead row has no evidence, as a fitted row with scale 0)
    const int hi = list_ptr[q + 1];
    for (int e = list_ptr[q] + threadIdx.x; e < hi; e += blockDim.x) {
        const int64_t id = list_ids[e];
        if (id >= 0 && id < n_src) atomicOr(&member[id], 1u << q);
    }
}

struct Epilogue {
    const double* scale;
    const double* prior;
    int64_t ld_prior;
    double coef, keep, lbd;            // keep = 1 - lbd
    int evidence;
};

__device__ inline double finish(const Epilogue& ep, double acc, unsigned cnt, int64_t b, int q) {
    const double sc = ep.scale[b];
    const double prod = sc * acc;
    double v;
    if (ep.evidence) {
        if (!(sc > 0.0)) cnt = 0;
        const double E = 1.0 - ldexp(1.0, -int(cnt < 255u ? cnt : 255u));
        v = ((ep.keep * E) * ep.coef) * prod;
    } else {
        v = ep.coef * prod;
    }
    if (ep.prior) v += ep.lbd * ep.prior[q * ep.ld_prior + b];
    return v;
}

// one entry of a row: a line of T (lane q's element) and, with evidence, the member word.  No branch: the loads of
// several entries are issued back to back (an id outside the source nodes reads line 0 and poisons the sum with NaN)
template <typename TT>
__device__ inline void take(const TT* __restrict__ T, const uint32_t* __restrict__ member, int64_t n_src, int j, int q,
                            TT& acc, unsigned& cnt) {
    const bool ok = j >= 0 && j < n_src;
    const int64_t jj = ok ? j : 0;
    const TT v = T[jj * kTile + q];
    acc += ok ? v : TT(__builtin_nanf(""));
    if (member) cnt += ok ? (member[jj] >> q) & 1u : 0u;
}

template <typename TT>
__global__ __launch_bounds__(256) void foldin_apply_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           int64_t n_out, int64_t n_src, const TT* __restrict__ T,
                                                           const uint32_t* __restrict__ member, int skip_long, Epilogue ep,
                                                           int n_tile, double* __restrict__ out, int64_t ld_out) {
    __shared__ double tile[kTile][33];
    __shared__ int skipped[32];
    const int q = threadIdx.x & 31, h = threadIdx.x >> 5;
    const int64_t b0 = int64_t(blockIdx.x) * 32;
    for (int i = 0; i < 4; ++i) {
        const int bl = h + 8 * i;
        const int64_t b = b0 + bl;
        double v = 0.0;
        int skip = 1;
        if (b < n_out) {
            const int lo = rowptr[b], hi = rowptr[b + 1];
            skip = skip_long && hi - lo > kLongRow;
            if (!skip) {
                TT a0 = 0, a1 = 0, a2 = 0, a3 = 0;
                unsigned cnt = 0;
                // 32 column ids per step, one coalesced load of the half wave, handed round by lane shuffles: the lines
                // of T they name are then independent loads (no id-then-line chain per entry).  Entry e goes to partial sum
                // (e - lo) % 4 in whole groups of four, the rest of the row to the first: a fixed order.
                for (int base = lo; base < hi; base += 32) {
                    const int mine = base + q < hi ? col[base + q] : 0;
                    const int m = hi - base < 32 ? hi - base : 32;
                    int t = 0;
                    for (; t + 4 <= m; t += 4) {
                        const int j0 = __shfl(mine, t, 32), j1 = __shfl(mine, t + 1, 32);
                        const int j2 = __shfl(mine, t + 2, 32), j3 = __shfl(mine, t + 3, 32);
                        take(T, member, n_src, j0, q, a0, cnt);
                        take(T, member, n_src, j1, q, a1, cnt);
                        take(T, member, n_src, j2, q, a2, cnt);
                        take(T, member, n_src, j3, q, a3, cnt);
                    }
                    for (; t < m; ++t) take(T, member, n_src, __shfl(mine, t, 32), q, a0, cnt);
                }
                v = finish(ep, double((a0 + a1) + (a2 + a3)), cnt, b, q < n_tile ? q : 0);
            }
        }
        tile[q][bl] = v;
        if (q == 0) skipped[bl] = skip;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < kTile * 32; idx += 256) {
        const int qq = idx >> 5, bl = idx & 31;
        const int64_t b = b0 + bl;
        if (qq < n_tile && b < n_out && !skipped[bl]) out[qq * ld_out + b] = tile[qq][bl];
    }
}

// A long row on one workgroup of 32 half waves: half wave h takes the groups of four entries h, h + 32, ... of the row
// (four independent lines in flight each, 128 per workgroup; entries past the end add zero), then the 32 partial sums are
// added in the order of h.
constexpr int kLongHalfWaves = 32;

template <typename TT>
__global__ __launch_bounds__(32 * kLongHalfWaves) void foldin_apply_long_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_out, int64_t n_src,
    const int32_t* __restrict__ long_rows, const TT* __restrict__ T, const uint32_t* __restrict__ member, Epilogue ep,
    int n_tile, double* __restrict__ out, int64_t ld_out) {
    __shared__ TT part[kLongHalfWaves][kTile];
    __shared__ unsigned pcnt[kLongHalfWaves][kTile];
    const int q = threadIdx.x & 31, h = threadIdx.x >> 5;
    const int64_t b = long_rows[blockIdx.x];
    if (b < 0 || b >= n_out) return;
    const int lo = rowptr[b], hi = rowptr[b + 1];
    TT a[4] = {0, 0, 0, 0};
    unsigned cnt = 0;
    for (int e = lo + 4 * h; e < hi; e += 4 * kLongHalfWaves) {
        int j[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) j[i] = e + i < hi ? col[e + i] : -1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool there = e + i < hi, ok = j[i] >= 0 && j[i] < n_src;
            const int64_t jj = there && ok ? j[i] : 0;
            const TT v = T[jj * kTile + q];
            a[i] += there ? (ok ? v : TT(__builtin_nanf(""))) : TT(0);
            if (member) cnt += there && ok ? (member[jj] >> q) & 1u : 0u;
        }
    }
    part[h][q] = (a[0] + a[1]) + (a[2] + a[3]);
    pcnt[h][q] = cnt;
    __syncthreads();
    if (h == 0 && q < n_tile) {
        TT acc = part[0][q];
        for (int p = 1; p < kLongHalfWaves; ++p) {
            acc += part[p][q];
            cnt += pcnt[p][q];
        }
        out[q * ld_out + b] = finish(ep, double(acc), cnt, b, q);
    }
}

template <int L>
void launch_gather(bool vec, unsigned grid, hipStream_t st, const void* S, int64_t stride, int64_t n_rows, int64_t n_cols,
                   const int32_t* col_ids, int64_t col_base, const int32_t* list_ptr, const int32_t* list_pos,
                   const double* w, int n_tile, void* T, int64_t n_src) {
    using A = typename Lay<L>::acc_t;
    if (vec)
        hipLaunchKernelGGL((foldin_gather_kernel<L, true>), dim3(grid), dim3(256), 0, st, S, stride, n_rows, n_cols, col_ids,
                           col_base, list_ptr, list_pos, w, n_tile, static_cast<A*>(T), n_src);
    else
        hipLaunchKernelGGL((foldin_gather_kernel<L, false>), dim3(grid), dim3(256), 0, st, S, stride, n_rows, n_cols, col_ids,
                           col_base, list_ptr, list_pos, w, n_tile, static_cast<A*>(T), n_src);
}

template <typename TT>
void launch_apply(hipStream_t st, const int32_t* rowptr, const int32_t* col, int64_t n_out, int64_t n_src,
                  const int32_t* long_rows, int64_t n_long, const void* T, const uint32_t* member, const Epilogue& ep,
                  int n_tile, double* out, int64_t ld_out) {
    const unsigned grid = (unsigned)((n_out + 31) / 32);
    hipLaunchKernelGGL(foldin_apply_kernel<TT>, dim3(grid), dim3(256), 0, st, rowptr, col, n_out, n_src,
                       static_cast<const TT*>(T), member, n_long > 0 ? 1 : 0, ep, n_tile, out, ld_out);
    if (n_long > 0)
        hipLaunchKernelGGL(foldin_apply_long_kernel<TT>, dim3((unsigned)n_long), dim3(32 * kLongHalfWaves), 0, st, rowptr, col, n_out, n_src,
                           long_rows, static_cast<const TT*>(T), member, ep, n_tile, out, ld_out);
}

}  // namespace

extern "C" {

int simrank_foldin_version(void) { return SIMRANK_FOLDIN_VERSION; }

const char* simrank_foldin_last_error(void) { return g_error.c_str(); }

int64_t simrank_foldin_t_bytes(int32_t layout, int64_t n_src) {
    if (!known_layout(layout) || n_src < 0) return -1;
    return n_src * kTile * int64_t(layout == SIMRANK_FOLDIN_ROWMAJOR_F64 ? sizeof(double) : sizeof(float));
}

int simrank_foldin_alloc(void** ptr, size_t bytes) {
    REQUIRE(ptr, "ptr is NULL");
    *ptr = nullptr;
    if (bytes == 0) return SIMRANK_FOLDIN_OK;
    HIP_CHECK(hipMalloc(ptr, bytes));
    return SIMRANK_FOLDIN_OK;
}

int simrank_foldin_free(void* ptr) {
    if (ptr) HIP_CHECK(hipFree(ptr));
    return SIMRANK_FOLDIN_OK;
}

int simrank_foldin_gather(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                          const int32_t* col_ids, int64_t col_base, const int32_t* list_ptr, const int32_t* list_pos,
                          const double* w, int32_t n_tile, void* T, int64_t n_src, void* stream) {
    REQUIRE(known_layout(layout), "unknown layout %d", (int)layout);
    REQUIRE(n_rows >= 0 && n_cols >= 0 && n_rows < (int64_t(1) << 31) && n_cols < (int64_t(1) << 31),
                "bad block shape %lld x %lld", (long long)n_rows, (long long)n_cols);
    REQUIRE(n_src >= 0 && n_src < (int64_t(1) << 31), "bad number of source nodes %lld", (long long)n_src);
    REQUIRE(n_tile >= 0 && n_tile <= kTile, "n_tile must be in [0, %d] (got %d)", kTile, (int)n_tile);
    const bool panels = is_panel(layout);
    REQUIRE(stride >= (panels ? n_rows : n_cols), "stride %lld is smaller than the block's %s (%lld)", (long long)stride,
                panels ? "rows" : "columns", (long long)(panels ? n_rows : n_cols));
    REQUIRE(col_ids || (col_base >= 0 && col_base + n_cols <= n_src), "columns %lld .. %lld are not source nodes",
                (long long)col_base, (long long)(col_base + n_cols));
    if (n_cols == 0 || n_src == 0) return SIMRANK_FOLDIN_OK;
    REQUIRE(S && T, "S or T is NULL");
    REQUIRE(n_tile == 0 || (list_ptr && w), "list_ptr or w is NULL");
    REQUIRE(reinterpret_cast<uintptr_t>(T) % 16 == 0, "T is not 16-byte aligned");
    const bool base16 = reinterpret_cast<uintptr_t>(S) % 16 == 0;
    REQUIRE(base16 || !panels, "a panel block starts on 16 bytes");
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        constexpr int K = Lay<L>::kCols, BC = 64 * K;                // a lane's run; the columns of one workgroup
        launch_gather<L>(panels || (base16 && stride % K == 0), (unsigned)((n_cols + BC - 1) / BC), st, S, stride, n_rows,
                         n_cols, col_ids, col_base, list_ptr, list_pos, w, n_tile, T, n_src);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_FOLDIN_OK;
}

int simrank_foldin_member(const int32_t* list_ptr, const int32_t* list_ids, const double* w, int32_t n_tile,
                          uint32_t* member, int64_t n_src, void* stream) {
    REQUIRE(n_src >= 0 && n_src < (int64_t(1) << 31), "bad number of source nodes %lld", (long long)n_src);
    REQUIRE(n_tile >= 0 && n_tile <= kTile, "n_tile must be in [0, %d] (got %d)", kTile, (int)n_tile);
    if (n_src == 0) return SIMRANK_FOLDIN_OK;
    REQUIRE(member, "member is NULL");
    REQUIRE(n_tile == 0 || (list_ptr && w), "list_ptr or w is NULL");
    hipStream_t st = as_stream(stream);
    HIP_CHECK(hipMemsetAsync(member, 0, sizeof(uint32_t) * size_t(n_src), st));
    if (n_tile > 0) {
        hipLaunchKernelGGL(foldin_member_kernel, dim3((unsigned)n_tile), dim3(256), 0, st, list_ptr, list_ids, w, member,
                           n_src);
        HIP_CHECK(hipGetLastError());
    }
    return SIMRANK_FOLDIN_OK;
}

int simrank_foldin_apply(const int32_t* rowptr, const int32_t* col, const double* scale, int64_t n_out, int64_t n_src,
                         const int32_t* long_rows, int64_t n_long, const void* T, int32_t t_layout, const uint32_t* member,
                         double coef, double lbd, const double* prior, int64_t ld_prior, int32_t n_tile, double* out,
                         int64_t ld_out, void* stream) {
    REQUIRE(known_layout(t_layout), "unknown layout %d", (int)t_layout);
    REQUIRE(n_out >= 0 && n_out < (int64_t(1) << 31) && n_src >= 0 && n_src < (int64_t(1) << 31),
                "bad shape %lld x %lld", (long long)n_out, (long long)n_src);
    REQUIRE(n_tile >= 0 && n_tile <= kTile, "n_tile must be in [0, %d] (got %d)", kTile, (int)n_tile);
    REQUIRE(n_long >= 0 && n_long <= n_out && (n_long == 0 || long_rows), "bad list of long rows");
    REQUIRE(ld_out >= n_out && (!prior || ld_prior >= n_out), "a leading dimension is smaller than the %lld fitted nodes",
                (long long)n_out);
    if (n_out == 0 || n_tile == 0) return SIMRANK_FOLDIN_OK;
    REQUIRE(rowptr && scale && out, "rowptr, scale or out is NULL");
    REQUIRE(T && n_src > 0, "T is NULL or there are no source nodes");
    Epilogue ep;
    ep.scale = scale;
    ep.prior = prior;
    ep.ld_prior = ld_prior;
    ep.coef = coef;
    ep.keep = 1.0 - lbd;
    ep.lbd = lbd;
    ep.evidence = member != nullptr;
    hipStream_t st = as_stream(stream);
    if (t_layout == SIMRANK_FOLDIN_ROWMAJOR_F64)
        launch_apply<double>(st, rowptr, col, n_out, n_src, long_rows, n_long, T, member, ep, n_tile, out, ld_out);
    else
        launch_apply<float>(st, rowptr, col, n_out, n_src, long_rows, n_long, T, member, ep, n_tile, out, ld_out);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_FOLDIN_OK;
}

}  // extern "C"
