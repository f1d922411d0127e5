// A kept model as a linear operator (include/simrank_operator.h, libsimrank_operator.so): S @ X and S.T @ X for a dense
// float64 X of at most 64 columns, S read IN PLACE from a block of the iterate in the layout its plan stores it.
//
//     product   a float64 GEMM whose left operand is never copied.  One workgroup owns kStrip = 128 output rows (a row
//               strip of S, or for the transposed product a column strip: in the panel layouts whole panels, each one
//               contiguous run of rows) and one PART of the contraction, and walks it in tiles of kDepth = 32: the tile
//               of S goes from global memory to registers with one 16-byte load per four elements (8 bytes of binary16,
//               2 x 16 of float64; element by element under a column map, at a ragged edge and where the block is not
//               aligned), is widened there and written to local memory contraction-major, A[k][m]; the tile of X
//               goes beside it.  The next tile's loads are issued before the current tile is multiplied.  A thread
//               holds 4 rows x TQ columns of the output (TQ = 4 or 8 for d <= 32, 64; d <= 8 takes the matrix-vector forms below): per step
//               4 + TQ eight-byte reads of local memory feed 4 x TQ fused multiply-adds; the 32 lanes that share a
//               column group read 32 consecutive doubles of A (no bank meets twice), the lanes that share rows read
//               the same words of X (a broadcast).
//               transpose = 0: eight lanes take the 128 bytes of a row's tile (in the panel layouts a wave's load is
//               1 KiB contiguous); a lane's four values go to four lines of A, a 2-way bank conflict on the store.
//               transpose = 1: 32 lanes take 512 contiguous bytes of a row; value i of lane c goes to A[k][32 i + c],
//               consecutive lanes to consecutive words, and the thread that owns the words 32 i + g owns the four
//               CONSECUTIVE output rows 4 g + i.
//     narrow    d <= 8: operator_rows_kernel and operator_cols_kernel keep S in registers; see there.
//     parts     the contraction is cut into P parts (a function of the shape, the direction and d alone: enough workgroups
//               to fill the device while a strip stays as it is), every workgroup writes its partial sums to the workspace, and
//     finish    adds the P partial sums of an element in the order of the parts and applies alpha and beta.  No
//               floating-point atomic anywhere: the order of every sum is fixed by the shape.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "simrank_operator.h"

#define COMPANION_ERR_INVALID SIMRANK_OPERATOR_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_OPERATOR_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_OPERATOR_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_OPERATOR_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_OPERATOR_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_OPERATOR_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int kStrip = SIMRANK_OPERATOR_STRIP;             // output rows of one workgroup
constexpr int kDepth = 32;                                 // steps of the contraction per tile
constexpr int kPitch = kStrip + 1;                         // doubles between two lines of A: odd, see the store
constexpr int kRows = 4;                                   // output rows of one thread
constexpr int kRowGroups = kStrip / kRows;                 // 32 lanes: the threads that share a column group
constexpr int kColGroups = kThreads / kRowGroups;          // 8
constexpr int kQuads = kStrip * kDepth / 4 / kThreads;     // quads of S one thread loads per tile
constexpr int kMaxParts = SIMRANK_OPERATOR_MAX_PARTS;
constexpr int64_t kWantGroups = 1536;                      // workgroups a call aims for: six per compute unit, whole rounds
                                                           // of the two (TQ = 8) or three workgroups a unit holds at once
static_assert(kStrip == 128 && kQuads == 4 && kColGroups * 8 == SIMRANK_OPERATOR_MAX_D, "the tile's geometry");

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
        for (int i = 0; i < 4; ++i) v[i] = (double)(__half2float(x.h[i]) * kHalfScale);
    } else {
        const double2* p = reinterpret_cast<const double2*>(static_cast<const double*>(S) + offset_of<L>(stride, r, c));
        const double2 a = p[0], b = p[1];
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    }
}

struct Block {
    const void* S;
    int64_t stride, n_rows, n_cols;
    const int32_t* row_pos;
    const int32_t* col_pos;
    int vec;                                               // no column map and every inner quad is one aligned vector load
};

// S[row(a)][col(b + i)] for i < 4 (b a multiple of 4): 0.0 past the end of either id range (it meets a 0.0 of X or an
// output row that is not stored), NaN for a position outside the block
template <int L>
__device__ __forceinline__ void fetch_quad(const Block& g, int64_t a, int64_t b, double (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = 0.0;
    if (a >= g.n_rows || b >= g.n_cols) return;
    const int64_t r = g.row_pos ? int64_t(g.row_pos[a]) : a;
    const double nan = __builtin_nan("");
    if (r < 0 || r >= g.n_rows) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (b + i < g.n_cols) v[i] = nan;
        return;
    }
    if (g.vec && b + 4 <= g.n_cols) {
        load_quad<L>(g.S, g.stride, r, b, v);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (b + i < g.n_cols) {
            const int64_t c = g.col_pos ? int64_t(g.col_pos[b + i]) : b + i;
            v[i] = c >= 0 && c < g.n_cols ? elem<L>(g.S, g.stride, r, c) : nan;
        }
    }
}

// part[p][m][q] = sum over part p of the contraction of S(m, k) * X[k][q].  T: the transposed product (m a column of S,
// k a row).  TQ: columns of one thread; the kernel serves d <= 8 TQ.  n_out / n_in: output rows and contraction length.
template <int L, bool T, int TQ>
__global__ __launch_bounds__(kThreads) void operator_product_kernel(Block g, int64_t n_out, int64_t n_in,
                                                                    const double* __restrict__ X, int64_t ld_x, int d,
                                                                    int64_t tiles_per_part, double* __restrict__ part) {
    constexpr int QW = kColGroups * TQ;                    // columns of the tile of X
    __shared__ double A[kDepth * kPitch];
    __shared__ double Xs[kDepth * QW];
    const int t = threadIdx.x;
    const int mg = t & (kRowGroups - 1), qg = t / kRowGroups;
    const int64_t m0 = int64_t(blockIdx.x) * kStrip;
    const int64_t n_tiles = (n_in + kDepth - 1) / kDepth;
    const int64_t tile_lo = int64_t(blockIdx.y) * tiles_per_part;
    const int64_t tile_hi = tile_lo + tiles_per_part < n_tiles ? tile_lo + tiles_per_part : n_tiles;

    double acc[kRows][TQ];
#pragma unroll
    for (int i = 0; i < kRows; ++i)
#pragma unroll
        for (int j = 0; j < TQ; ++j) acc[i][j] = 0.0;

    double pa[kQuads][4], px[TQ];                          // the next tile, on its way from global memory
    auto fetch = [&](int64_t tile) {
        const int64_t k0 = tile * kDepth;
#pragma unroll
        for (int u = 0; u < kQuads; ++u) {
            const int idx = t + u * kThreads;
            if constexpr (!T) fetch_quad<L>(g, m0 + (idx >> 3), k0 + (idx & 7) * 4, pa[u]);
            else fetch_quad<L>(g, k0 + (idx >> 5), m0 + (idx & 31) * 4, pa[u]);
        }
#pragma unroll
        for (int u = 0; u < TQ; ++u) {
            const int idx = t + u * kThreads;
            const int64_t k = k0 + idx / QW;
            const int q = idx % QW;
            px[u] = k < n_in && q < d ? X[k * ld_x + q] : 0.0;
        }
    };

    if (tile_lo < tile_hi) fetch(tile_lo);
    for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
        __syncthreads();                                   // (the previous tile has been multiplied)
#pragma unroll
        for (int u = 0; u < kQuads; ++u) {
            const int idx = t + u * kThreads;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (!T) A[((idx & 7) * 4 + i) * kPitch + (idx >> 3)] = pa[u][i];
                else A[(idx >> 5) * kPitch + i * 32 + (idx & 31)] = pa[u][i];
            }
        }
#pragma unroll
        for (int u = 0; u < TQ; ++u) Xs[t + u * kThreads] = px[u];
        __syncthreads();
        if (tile + 1 < tile_hi) fetch(tile + 1);
#pragma unroll 4
        for (int k = 0; k < kDepth; ++k) {
            double a[kRows], x[TQ];
#pragma unroll
            for (int i = 0; i < kRows; ++i) a[i] = A[k * kPitch + i * kRowGroups + mg];
#pragma unroll
            for (int j = 0; j < TQ; ++j) x[j] = Xs[k * QW + qg * TQ + j];
#pragma unroll
            for (int i = 0; i < kRows; ++i)
#pragma unroll
                for (int j = 0; j < TQ; ++j) acc[i][j] = fma(a[i], x[j], acc[i][j]);
        }
    }

    double* __restrict__ mine = part + int64_t(blockIdx.y) * n_out * d;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
        const int64_t m = m0 + (T ? mg * kRows + i : i * kRowGroups + mg);
        if (m >= n_out) continue;
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const int q = qg * TQ + j;
            if (q < d) mine[m * d + q] = acc[i][j];
        }
    }
}

// ---- d <= 8: the matrix-vector forms.  One column of X lets a lane keep its elements of S in registers, so S does not go
// through local memory at all; only the tile of X does.
constexpr int kNarrow = SIMRANK_OPERATOR_NARROW;           // columns of X the two kernels below serve (padded with 0.0 to it)
constexpr int kRowsStrip = 16;                             // transpose = 0: output rows of one workgroup, 4 per wave
constexpr int kRowsDepth = 256;                            //   steps of the contraction per tile: a quad per lane
constexpr int kColsStrip = 4 * kThreads;                   // transpose = 1: output rows of one workgroup, a quad per lane
constexpr int kColsDepth = 64;                             //   steps of the contraction per tile
static_assert(kNarrow == 8 && kColsStrip == 1024, "the narrow forms' geometry");

// transpose = 0.  A wave carries four rows of S; per tile a lane loads one quad of each (the wave: 1 KiB of each row),
// and multiplies them by its four rows of the tile of X, which lies transposed in local memory (Xs[q][k]: a lane reads 32
// consecutive bytes, the wave 2 KiB: no bank meets twice).  The 64 partial sums of a row are added by an xor butterfly.
template <int L>
__global__ __launch_bounds__(kThreads) void operator_rows_kernel(Block g, int64_t n_out, int64_t n_in,
                                                                 const double* __restrict__ X, int64_t ld_x, int d,
                                                                 int64_t tiles_per_part, double* __restrict__ part) {
    constexpr int R = kRowsStrip / (kThreads / 64);
    __shared__ __attribute__((aligned(16))) double Xs[kNarrow][kRowsDepth];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t a0 = int64_t(blockIdx.x) * kRowsStrip + wave * R;
    const int64_t n_tiles = (n_in + kRowsDepth - 1) / kRowsDepth;
    const int64_t tile_lo = int64_t(blockIdx.y) * tiles_per_part;
    const int64_t tile_hi = tile_lo + tiles_per_part < n_tiles ? tile_lo + tiles_per_part : n_tiles;
    double acc[R][kNarrow];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < kNarrow; ++q) acc[r][q] = 0.0;
    for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
        const int64_t k0 = tile * kRowsDepth;
        double s[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r) fetch_quad<L>(g, a0 + r, k0 + lane * 4, s[r]);
        __syncthreads();                                   // (the previous tile of X has been read)
        {
            const int64_t k = k0 + t;
#pragma unroll
            for (int q = 0; q < kNarrow; ++q) Xs[q][t] = k < n_in && q < d ? X[k * ld_x + q] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kNarrow; ++q) {
            const double2 x01 = *reinterpret_cast<const double2*>(&Xs[q][lane * 4]);
            const double2 x23 = *reinterpret_cast<const double2*>(&Xs[q][lane * 4 + 2]);
#pragma unroll
            for (int r = 0; r < R; ++r)
                acc[r][q] = fma(s[r][3], x23.y, fma(s[r][2], x23.x, fma(s[r][1], x01.y, fma(s[r][0], x01.x, acc[r][q]))));
        }
    }
    double* __restrict__ mine = part + int64_t(blockIdx.y) * n_out * d;
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int q = 0; q < kNarrow; ++q) {
            double v = acc[r][q];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0 && a0 + r < n_out && q < d) mine[(a0 + r) * d + q] = v;
        }
    }
}

// transpose = 1.  A lane owns four consecutive output rows (columns of S) and walks the rows of S: one quad per row (the
// wave: 1 KiB contiguous in a row-major row, 128-byte pieces of 8 or 4 panels), times that row of X, which every lane
// reads from the same words of local memory (a broadcast).  No sum crosses a lane.
template <int L>
__global__ __launch_bounds__(kThreads) void operator_cols_kernel(Block g, int64_t n_out, int64_t n_in,
                                                                 const double* __restrict__ X, int64_t ld_x, int d,
                                                                 int64_t tiles_per_part, double* __restrict__ part) {
    constexpr int U = 4;                                   // rows of S in flight per lane
    __shared__ double Xs[kColsDepth][kNarrow];
    const int t = threadIdx.x;
    const int64_t b0 = int64_t(blockIdx.x) * kColsStrip + t * 4;
    const int64_t n_tiles = (n_in + kColsDepth - 1) / kColsDepth;
    const int64_t tile_lo = int64_t(blockIdx.y) * tiles_per_part;
    const int64_t tile_hi = tile_lo + tiles_per_part < n_tiles ? tile_lo + tiles_per_part : n_tiles;
    double acc[4][kNarrow];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < kNarrow; ++q) acc[i][q] = 0.0;
    for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
        const int64_t k0 = tile * kColsDepth;
        __syncthreads();                                   // (the previous tile of X has been read)
#pragma unroll
        for (int u = 0; u < kColsDepth * kNarrow / kThreads; ++u) {
            const int idx = t + u * kThreads;
            const int64_t k = k0 + idx / kNarrow;
            const int q = idx % kNarrow;
            Xs[idx / kNarrow][q] = k < n_in && q < d ? X[k * ld_x + q] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < kColsDepth; kk += U) {
            double s[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) fetch_quad<L>(g, k0 + kk + u, b0, s[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < kNarrow; ++q) {
                    const double x = Xs[kk + u][q];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i][q] = fma(s[u][i], x, acc[i][q]);
                }
        }
    }
    double* __restrict__ mine = part + int64_t(blockIdx.y) * n_out * d;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (b0 + i >= n_out) continue;
#pragma unroll
        for (int q = 0; q < kNarrow; ++q)
            if (q < d) mine[(b0 + i) * d + q] = acc[i][q];
    }
}

// out[m][q] = alpha * (part[0][m][q] + part[1][m][q] + ...) + beta * out[m][q]; beta == 0: out is not read
__global__ __launch_bounds__(kThreads) void operator_finish_kernel(const double* __restrict__ part, int parts, int64_t n_out,
                                                                   int d, double alpha, double beta,
                                                                   double* __restrict__ out, int64_t ld_out) {
    const int64_t idx = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    const int64_t total = n_out * d;
    if (idx >= total) return;
    double s = part[idx];
    for (int p = 1; p < parts; ++p) s += part[int64_t(p) * total + idx];
    double* o = out + (idx / d) * ld_out + idx % d;
    *o = beta == 0.0 ? alpha * s : alpha * s + beta * *o;
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct Plan {
    int64_t n_out, n_in, strips, tiles_per_part;
    int parts, narrow;
};

// strips, tiles and parts of a call: a function of the shape, the direction and d alone
bool plan_of(int64_t n_rows, int64_t n_cols, int32_t transpose, int32_t d, Plan* p) {
    if (n_rows < 0 || n_cols < 0 || n_rows >= (int64_t(1) << 31) || n_cols >= (int64_t(1) << 31)) return false;
    if (transpose != 0 && transpose != 1) return false;
    if (d < 1 || d > SIMRANK_OPERATOR_MAX_D) return false;
    p->narrow = d <= kNarrow;
    const int64_t strip = !p->narrow ? kStrip : transpose ? kColsStrip : kRowsStrip;
    const int64_t depth = !p->narrow ? kDepth : transpose ? kColsDepth : kRowsDepth;
    p->n_out = transpose ? n_cols : n_rows;
    p->n_in = transpose ? n_rows : n_cols;
    p->strips = (p->n_out + strip - 1) / strip;
    const int64_t tiles = (p->n_in + depth - 1) / depth;
    int64_t parts = p->strips ? (kWantGroups + p->strips - 1) / p->strips : 1;
    parts = std::max<int64_t>(1, std::min<int64_t>({parts, tiles, int64_t(kMaxParts)}));
    p->tiles_per_part = std::max<int64_t>(1, (tiles + parts - 1) / parts);
    p->parts = (int)std::max<int64_t>(1, (tiles + p->tiles_per_part - 1) / p->tiles_per_part);     // (no empty part)
    return true;
}

template <int L, bool T>
void launch_product(int d, dim3 grid, hipStream_t st, const Block& g, const Plan& p, const double* X, int64_t ld_x,
                    double* part) {
    if (d <= 32)
        hipLaunchKernelGGL((operator_product_kernel<L, T, 4>), grid, dim3(kThreads), 0, st, g, p.n_out, p.n_in, X, ld_x, d,
                           p.tiles_per_part, part);
    else
        hipLaunchKernelGGL((operator_product_kernel<L, T, 8>), grid, dim3(kThreads), 0, st, g, p.n_out, p.n_in, X, ld_x, d,
                           p.tiles_per_part, part);
}

}  // namespace

extern "C" {

int simrank_operator_version(void) { return SIMRANK_OPERATOR_VERSION; }

const char* simrank_operator_last_error(void) { return g_error.c_str(); }

int64_t simrank_operator_parts(int64_t n_rows, int64_t n_cols, int32_t transpose, int32_t d) {
    Plan p;
    return plan_of(n_rows, n_cols, transpose, d, &p) ? p.parts : -1;
}

int64_t simrank_operator_workspace_bytes(int64_t n_rows, int64_t n_cols, int32_t transpose, int32_t d) {
    Plan p;
    if (!plan_of(n_rows, n_cols, transpose, d, &p)) return -1;
    return std::max<int64_t>(8, int64_t(p.parts) * p.n_out * d * 8);
}

int simrank_operator_apply(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                           const int32_t* row_pos, const int32_t* col_pos, int32_t transpose, const double* X, int64_t ld_x,
                           int32_t d, double alpha, double beta, double* out, int64_t ld_out, void* workspace,
                           void* stream) {
    const int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    REQUIRE(transpose == 0 || transpose == 1, "transpose must be 0 or 1 (got %d)", (int)transpose);
    REQUIRE(d >= 1 && d <= SIMRANK_OPERATOR_MAX_D, "d must lie in 1 .. %d (got %d): cut a wider X into bands",
            SIMRANK_OPERATOR_MAX_D, (int)d);
    REQUIRE(ld_x >= d && ld_out >= d, "a leading dimension (%lld, %lld) is smaller than d = %d", (long long)ld_x,
            (long long)ld_out, (int)d);
    Plan p;
    REQUIRE(plan_of(n_rows, n_cols, transpose, d, &p), "bad block shape %lld x %lld", (long long)n_rows, (long long)n_cols);
    if (p.n_out == 0) return SIMRANK_OPERATOR_OK;
    REQUIRE(out && workspace, "out or workspace is NULL");
    REQUIRE(X || p.n_in == 0, "X is NULL");
    REQUIRE(reinterpret_cast<uintptr_t>(X) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
            "X, out and workspace must be 8-byte aligned");
    const Block g{S, stride, n_rows, n_cols, row_pos, col_pos, !col_pos && quad_vector_loads(S, layout, stride)};
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)p.strips, (unsigned)p.parts);
    double* part = static_cast<double*>(workspace);
    with_layout(layout, [&](auto L) {
        if (p.narrow && transpose)
            hipLaunchKernelGGL((operator_cols_kernel<L>), grid, dim3(kThreads), 0, st, g, p.n_out, p.n_in, X, ld_x, (int)d,
                               p.tiles_per_part, part);
        else if (p.narrow)
            hipLaunchKernelGGL((operator_rows_kernel<L>), grid, dim3(kThreads), 0, st, g, p.n_out, p.n_in, X, ld_x, (int)d,
                               p.tiles_per_part, part);
        else if (transpose) launch_product<L, true>(d, grid, st, g, p, X, ld_x, part);
        else launch_product<L, false>(d, grid, st, g, p, X, ld_x, part);
    });
    HIP_CHECK(hipGetLastError());
    const int64_t total = p.n_out * d;
    hipLaunchKernelGGL(operator_finish_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       part, p.parts, p.n_out, (int)d, alpha, beta, out, ld_out);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_OPERATOR_OK;
}

}  // extern "C"
