// Basket queries on an iterate that stays on the device (include/simrank_sets.h, libsimrank_sets.so): the weighted sum
// of a set of rows, read IN PLACE from a block of the iterate in the layout its plan stores it, and the k best of it.
//
//     score   out[q][j] = sum_e w_e * S[pos_e][col(j)], float64, in list order, product and sum rounded separately.  A
//             basket of m members reads m lines per lane and writes one, so the kernel is shaped by its READS: a
//             workgroup owns one basket and 1024 consecutive output columns, a lane owns 4 of them and keeps their four
//             float64 sums in registers while it walks the member list.  Without a column map those 4 columns are 16
//             contiguous bytes of an f32 row or panel (8 of a binary16 panel, 32 of a float64 row): one vector load per
//             member, kUnroll members' loads issued before the first is consumed.  With a column map (a kept plan whose
//             order is not the caller's) the 4 columns are gathered one by one, as query_rows_kernel gathers them.
//             The member list is uniform over the workgroup: its positions and weights come through scalar loads.
//     topk    one wave per row of the float64 band, k rounds of "largest element after the previous pick" in the total
//             order (value descending, id ascending), as query_topk_kernel; -inf (an excluded column) and NaN are no
//             candidates.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "simrank_sets.h"

#define COMPANION_ERR_INVALID SIMRANK_SETS_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_SETS_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_SETS_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_SETS_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_SETS_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_SETS_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int kPerThread = 4;                              // output columns of one lane
constexpr int kChunk = kThreads * kPerThread;              // output columns of one workgroup
constexpr int kUnroll = 8;                                 // members whose loads are in flight together
static_assert(kChunk == SIMRANK_SETS_CHUNK, "the header's chunk is the kernel's");

// acc + (w * s) with both roundings: the compiler may not contract the two into a fused multiply-add
__device__ __forceinline__ double add_product(double acc, double w, double s) {
#pragma clang fp contract(off)
    const double p = w * s;
    return acc + p;
}

// four consecutive columns c .. c + 3 (c a multiple of 4) of row r, widened; the 16 / 8 / 32 bytes are contiguous
struct Quad {
    double v[kPerThread];
};

template <int L>
__device__ __forceinline__ Quad load_quad(const void* __restrict__ S, int64_t stride, int64_t r, int64_t c) {
    Quad q;
    if constexpr (L == PANEL_F32 || L == ROWMAJOR_F32) {
        const int64_t at = L == PANEL_F32 ? ((c >> 5) * stride + r) * 32 + (c & 31) : r * stride + c;
        const float4 x = *reinterpret_cast<const float4*>(static_cast<const float*>(S) + at);
        q.v[0] = (double)x.x, q.v[1] = (double)x.y, q.v[2] = (double)x.z, q.v[3] = (double)x.w;
    } else if constexpr (L == PANEL_F16) {
        const int64_t at = ((c >> 6) * stride + r) * 64 + (c & 63);
        union {
            uint2 bits;
            __half h[4];
        } x;
        x.bits = *reinterpret_cast<const uint2*>(static_cast<const __half*>(S) + at);
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) q.v[i] = (double)(__half2float(x.h[i]) * kHalfScale);
    } else {
        const double2* p = reinterpret_cast<const double2*>(static_cast<const double*>(S) + r * stride + c);
        const double2 a = p[0], b = p[1];
        q.v[0] = a.x, q.v[1] = a.y, q.v[2] = b.x, q.v[3] = b.y;
    }
    return q;
}

// The workgroup's basket and chunk.  Basket-major: consecutive workgroups walk the chunks of one basket.  Chunk-label:
// block b has label x = b % 8 (the blocks that share an XCD) and slot b / 8; with 8 chunks or more, label x owns the
// chunks x, x + 8, ... and its slots walk (basket, own chunk); with fewer, chunk c owns the labels c, c + chunks, ... and
// the baskets are dealt among them.
__device__ __forceinline__ bool place(int grid_order, int64_t b, int64_t n_sets, int64_t chunks, int64_t& q, int64_t& chunk) {
    if (grid_order == SIMRANK_SETS_GRID_BASKET_MAJOR) {
        q = b / chunks;
        chunk = b % chunks;
        return q < n_sets;
    }
    const int64_t x = b & 7, slot = b >> 3;
    if (chunks >= 8) {
        const int64_t per = (chunks + 7) >> 3;
        q = slot / per;
        chunk = x + ((slot % per) << 3);
    } else {
        chunk = x % chunks;
        const int64_t labels = (7 - chunk) / chunks + 1;
        q = slot * labels + x / chunks;
    }
    return q < n_sets && chunk < chunks;
}

// VEC: no column map, every quad of a full lane is one aligned vector load.  Otherwise element by element through
// col_pos (or the block's own order when col_pos is NULL and the block is not aligned for vector loads).
template <int L, bool VEC>
__global__ __launch_bounds__(kThreads) void sets_score_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                              int64_t n_cols, const int32_t* __restrict__ col_pos,
                                                              int64_t n_out, const int64_t* __restrict__ set_ptr,
                                                              const int32_t* __restrict__ set_pos,
                                                              const double* __restrict__ set_w, int64_t n_sets,
                                                              const int64_t* __restrict__ excl_ptr,
                                                              const int32_t* __restrict__ excl_cols, int64_t chunks,
                                                              int grid_order, double* __restrict__ out, int64_t ld_out) {
    int64_t q, chunk;
    if (!place(grid_order, blockIdx.x, n_sets, chunks, q, chunk)) return;
    const int64_t j0 = chunk * kChunk + int64_t(threadIdx.x) * kPerThread;
    if (j0 >= n_out) return;
    const int64_t e0 = set_ptr[q], e1 = set_ptr[q + 1];
    const double nan = __builtin_nan("");
    double acc[kPerThread] = {0.0, 0.0, 0.0, 0.0};

    if (VEC && j0 + kPerThread <= n_out) {
        int64_t e = e0;
        for (; e + kUnroll <= e1; e += kUnroll) {
            Quad x[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int64_t r = set_pos[e + u];
                x[u] = (r >= 0 && r < n_rows) ? load_quad<L>(S, stride, r, j0) : Quad{{nan, nan, nan, nan}};
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const double w = set_w[e + u];
#pragma unroll
                for (int i = 0; i < kPerThread; ++i) acc[i] = add_product(acc[i], w, x[u].v[i]);
            }
        }
        for (; e < e1; ++e) {
            const int64_t r = set_pos[e];
            const double w = set_w[e];
            const Quad x = (r >= 0 && r < n_rows) ? load_quad<L>(S, stride, r, j0) : Quad{{nan, nan, nan, nan}};
#pragma unroll
            for (int i = 0; i < kPerThread; ++i) acc[i] = add_product(acc[i], w, x.v[i]);
        }
    } else {
        // the lane's source columns, once: -1 = past the output or outside the block (never read)
        int64_t c[kPerThread];
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) {
            const int64_t j = j0 + i;
            c[i] = -1;
            if (j < n_out) {
                const int64_t cc = col_pos ? int64_t(col_pos[j]) : j;
                if (cc >= 0 && cc < n_cols) c[i] = cc;
            }
        }
        int64_t e = e0;
        for (; e + kUnroll <= e1; e += kUnroll) {
            double x[kUnroll][kPerThread];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int64_t r = set_pos[e + u];
                const bool ok = r >= 0 && r < n_rows;
#pragma unroll
                for (int i = 0; i < kPerThread; ++i) x[u][i] = (ok && c[i] >= 0) ? elem<L>(S, stride, r, c[i]) : nan;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const double w = set_w[e + u];
#pragma unroll
                for (int i = 0; i < kPerThread; ++i) acc[i] = add_product(acc[i], w, x[u][i]);
            }
        }
        for (; e < e1; ++e) {
            const int64_t r = set_pos[e];
            const double w = set_w[e];
            const bool ok = r >= 0 && r < n_rows;
#pragma unroll
            for (int i = 0; i < kPerThread; ++i)
                acc[i] = add_product(acc[i], w, (ok && c[i] >= 0) ? elem<L>(S, stride, r, c[i]) : nan);
        }
    }

    // the basket's excluded output columns that are this lane's
    if (excl_ptr) {
        const int64_t x1 = excl_ptr[q + 1];
        for (int64_t x = excl_ptr[q]; x < x1; ++x) {
            const int64_t d = int64_t(excl_cols[x]) - j0;
#pragma unroll
            for (int i = 0; i < kPerThread; ++i)
                if (d == i) acc[i] = -__builtin_inf();
        }
    }
    double* o = out + q * ld_out + j0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i)
        if (j0 + i < n_out) o[i] = acc[i];
}

__global__ __launch_bounds__(256) void sets_topk_kernel(const double* __restrict__ band, int64_t ld_band, int64_t n_sets,
                                                        int64_t n_out, const int32_t* __restrict__ col_ids, int k,
                                                        int32_t* __restrict__ idx_out, double* __restrict__ val_out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    const double ninf = -__builtin_inf();
    for (int64_t q = wave; q < n_sets; q += nwaves) {
        const double* row = band + q * ld_band;
        double pv = __builtin_inf();        // previous pick: everything is "after" (+inf, -1)
        int pi = -1;
        int j = 0;
        for (; j < k; ++j) {
            double bv = ninf;
            int bi = 0x7fffffff;
            for (int64_t c = lane; c < n_out; c += 64) {
                const double v = row[c];
                const int id = col_ids ? col_ids[c] : int(c);
                const bool after = (v < pv) || (v == pv && id > pi);
                const bool better = (v > bv) || (v == bv && id < bi);
                if (v > ninf && after && better) { bv = v; bi = id; }     // (v > -inf: false for NaN too)
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                if ((ov > bv) || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (bi == 0x7fffffff) break;
            if (lane == 0) {
                idx_out[q * k + j] = bi;
                val_out[q * k + j] = bv;
            }
            pv = bv;
            pi = bi;
        }
        for (int jj = j + lane; jj < k; jj += 64) {
            idx_out[q * k + jj] = -1;
            val_out[q * k + jj] = 0.0;
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
int64_t grid_blocks(int64_t n_sets, int64_t n_out, int32_t grid_order) {
    if (n_sets < 0 || n_out < 0 || n_sets >= (int64_t(1) << 31) || n_out >= (int64_t(1) << 31)) return -1;
    if (grid_order != SIMRANK_SETS_GRID_BASKET_MAJOR && grid_order != SIMRANK_SETS_GRID_CHUNK_LABEL) return -1;
    if (n_sets == 0 || n_out == 0) return 0;
    const int64_t chunks = (n_out + kChunk - 1) / kChunk;
    if (grid_order == SIMRANK_SETS_GRID_BASKET_MAJOR) return n_sets * chunks;
    if (chunks >= 8) return 8 * n_sets * ((chunks + 7) / 8);
    const int64_t fewest = 8 / chunks;                   // labels of the chunk that has the fewest
    return 8 * ((n_sets + fewest - 1) / fewest);
}

template <int L>
void launch_score(bool vec, dim3 grid, hipStream_t st, const void* S, int64_t stride, int64_t n_rows, int64_t n_cols,
                  const int32_t* col_pos, int64_t n_out, const int64_t* set_ptr, const int32_t* set_pos,
                  const double* set_w, int64_t n_sets, const int64_t* excl_ptr, const int32_t* excl_cols, int64_t chunks,
                  int grid_order, double* out, int64_t ld_out) {
    if (vec)
        hipLaunchKernelGGL((sets_score_kernel<L, true>), grid, dim3(kThreads), 0, st, S, stride, n_rows, n_cols, col_pos,
                           n_out, set_ptr, set_pos, set_w, n_sets, excl_ptr, excl_cols, chunks, grid_order, out, ld_out);
    else
        hipLaunchKernelGGL((sets_score_kernel<L, false>), grid, dim3(kThreads), 0, st, S, stride, n_rows, n_cols, col_pos,
                           n_out, set_ptr, set_pos, set_w, n_sets, excl_ptr, excl_cols, chunks, grid_order, out, ld_out);
}

}  // namespace

extern "C" {

int simrank_sets_version(void) { return SIMRANK_SETS_VERSION; }

const char* simrank_sets_last_error(void) { return g_error.c_str(); }

int64_t simrank_sets_blocks(int64_t n_sets, int64_t n_out, int32_t grid_order) {
    return grid_blocks(n_sets, n_out, grid_order);
}

int simrank_sets_score(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols,
                       const int32_t* col_pos, int64_t n_out, const int64_t* set_ptr, const int32_t* set_pos,
                       const double* set_w, int64_t n_sets, const int64_t* excl_ptr, const int32_t* excl_cols,
                       double* out, int64_t ld_out, int32_t grid_order, void* stream) {
    const int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    REQUIRE(n_sets >= 0 && n_out >= 0 && ld_out >= n_out, "bad output shape %lld x %lld (ld %lld)", (long long)n_sets,
            (long long)n_out, (long long)ld_out);
    REQUIRE(col_pos || n_out <= n_cols, "n_out %lld exceeds the block's %lld columns and there is no column map",
            (long long)n_out, (long long)n_cols);
    REQUIRE((excl_ptr == nullptr) == (excl_cols == nullptr), "excl_ptr and excl_cols go together");
    const int64_t blocks = grid_blocks(n_sets, n_out, grid_order);
    REQUIRE(blocks >= 0, "bad grid order %d or sizes", (int)grid_order);
    REQUIRE(blocks <= SIMRANK_SETS_MAX_BLOCKS, "%lld baskets x %lld columns are too many for one call (%lld workgroups): "
            "cut the baskets into bands", (long long)n_sets, (long long)n_out, (long long)blocks);
    if (blocks == 0) return SIMRANK_SETS_OK;
    REQUIRE(set_ptr && out, "set_ptr or out is NULL");
    // (set_pos and set_w may be NULL when every basket is empty: they are then never read)
    const int64_t chunks = (n_out + kChunk - 1) / kChunk;
    const bool vec = !col_pos && quad_vector_loads(S, layout, stride);
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)blocks);
    with_layout(layout, [&](auto L) {
        launch_score<L>(vec, grid, st, S, stride, n_rows, n_cols, col_pos, n_out, set_ptr, set_pos, set_w, n_sets, excl_ptr,
                        excl_cols, chunks, (int)grid_order, out, ld_out);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_SETS_OK;
}

int simrank_sets_topk(const double* band, int64_t ld_band, int64_t n_sets, int64_t n_out, const int32_t* col_ids, int32_t k,
                      int32_t* idx_out, double* val_out, void* stream) {
    REQUIRE(n_sets >= 0 && n_sets < (int64_t(1) << 31) && n_out >= 0 && n_out < (int64_t(1) << 31) && ld_band >= n_out,
            "bad band shape %lld x %lld (ld %lld)", (long long)n_sets, (long long)n_out, (long long)ld_band);
    REQUIRE(k >= 1, "k must be positive (got %d)", (int)k);
    REQUIRE(int64_t(k) * n_sets < (int64_t(1) << 40), "k x rows is too large");
    if (n_sets == 0) return SIMRANK_SETS_OK;
    REQUIRE(idx_out && val_out, "idx_out or val_out is NULL");
    REQUIRE(band || n_out == 0, "band is NULL");
    hipStream_t st = as_stream(stream);
    const unsigned grid = (unsigned)std::min<int64_t>((n_sets + 3) / 4, int64_t(1) << 16);
    hipLaunchKernelGGL(sets_topk_kernel, dim3(grid), dim3(256), 0, st, band, ld_band, n_sets, n_out, col_ids, (int)k, idx_out,
                       val_out);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_SETS_OK;
}

}  // extern "C"
