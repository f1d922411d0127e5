// Node queries on an iterate that stays on the device (include/simrank_query.h, libsimrank_query.so): chosen rows,
// chosen pairs and the k best of chosen rows, read IN PLACE from a block of the iterate in the layout its plan stores it
// (f32 32-column panels, f32 row-major shard blocks, fp16-held 64-column panels, float64 row-major) and widened to
// double on the device the way the dense hand-back widens them, so every queried value is bit-identical to the same
// element of the dense result.
//
//     rows    out[q][j] = S[row_pos[q]][col_pos[j]].  The output is what costs: 8 bytes written per 4 or 2 read.  So the
//             kernel is shaped by its stores — a workgroup writes 1024 consecutive doubles of one query row, 8 bytes per
//             lane, 512 contiguous bytes per wave instruction, four independent elements per thread in flight — and
//             GATHERS the sources: the column map (solver's order -> caller's) scatters a row's elements over its
//             128-byte panel segments, but the whole row is 2 or 4 bytes x n_cols (128 KiB at N = 32768 in f32), a small
//             part of one XCD's L2.  All workgroups of a query row carry the same blockIdx % 8, the label of the blocks
//             that share an XCD, so each segment comes from HBM once and the other gathers of that row hit in L2.
//             (Staging the row in LDS with 16-byte reads would serve a row of at most 160 KiB, one workgroup per CU, and
//             scattering 8-byte stores instead would write partial lines: neither pays against gathers that hit L2.)
//     pairs   one element per thread.
//     topk    one wave per query row, k rounds of "largest element after the previous pick" in the total order (value
//             descending, id ascending), the row's own node excluded by ID — the order and the empty-slot convention of
//             the main library's top-k, on any subset of rows; the row is re-read from L2.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "simrank_query.h"

#define COMPANION_ERR_INVALID SIMRANK_QUERY_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_QUERY_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_QUERY_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_QUERY_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_QUERY_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_QUERY_, ROWMAJOR_F64);

constexpr int kRowsThreads = 256;
constexpr int kRowsPerThread = 4;
constexpr int kRowsChunk = kRowsThreads * kRowsPerThread;      // output columns of one workgroup

// Block b: label x = b % 8 (the blocks that share an XCD), slot s = b / 8; the slots of a label walk the chunks of the
// query rows q = 8 * (s / chunks) + x, so that every chunk of a query row runs under the same label.
template <int L>
__global__ __launch_bounds__(kRowsThreads) void query_rows_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                                  int64_t n_cols, const int32_t* __restrict__ row_pos,
                                                                  int64_t n_q, const int32_t* __restrict__ col_pos,
                                                                  int64_t n_out, int64_t chunks, double* __restrict__ out,
                                                                  int64_t ld_out) {
    const int64_t b = blockIdx.x;
    const int64_t slot = b >> 3;
    const int64_t q = ((slot / chunks) << 3) + (b & 7);
    if (q >= n_q) return;
    const int64_t j0 = (slot % chunks) * kRowsChunk + threadIdx.x;
    const int64_t r = row_pos[q];
    const bool row_ok = r >= 0 && r < n_rows;
    double v[kRowsPerThread];
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
        const int64_t j = j0 + int64_t(i) * kRowsThreads;
        v[i] = __builtin_nan("");
        if (j < n_out) {
            const int64_t c = col_pos ? int64_t(col_pos[j]) : j;
            if (row_ok && c >= 0 && c < n_cols) v[i] = elem<L>(S, stride, r, c);
        }
    }
    double* o = out + q * ld_out;
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
        const int64_t j = j0 + int64_t(i) * kRowsThreads;
        if (j < n_out) o[j] = v[i];
    }
}

template <int L>
__global__ __launch_bounds__(256) void query_pairs_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                          int64_t n_cols, const int32_t* __restrict__ a_pos,
                                                          const int32_t* __restrict__ b_pos, int64_t n_pairs,
                                                          double* __restrict__ out) {
    const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (i >= n_pairs) return;
    const int64_t r = a_pos[i], c = b_pos[i];
    out[i] = (r >= 0 && r < n_rows && c >= 0 && c < n_cols) ? elem<L>(S, stride, r, c) : __builtin_nan("");
}

template <int L>
__global__ __launch_bounds__(256) void query_topk_kernel(const void* __restrict__ S, int64_t stride, int64_t n_rows,
                                                         int64_t n_cols, const int32_t* __restrict__ row_pos,
                                                         const int32_t* __restrict__ row_ids, int64_t n_q,
                                                         const int32_t* __restrict__ col_ids, int k,
                                                         int32_t* __restrict__ idx_out, double* __restrict__ val_out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t q = wave; q < n_q; q += nwaves) {
        const int64_t r = row_pos[q];
        const int self = row_ids[q];
        const int64_t cols = (r >= 0 && r < n_rows) ? n_cols : 0;       // (a row outside the block: no candidates)
        double pv = __builtin_inf();        // previous pick: everything is "after" (+inf, -1)
        int pi = -1;
        int j = 0;
        for (; j < k; ++j) {
            double bv = -__builtin_inf();
            int bi = 0x7fffffff;
            for (int64_t c = lane; c < cols; c += 64) {
                const double v = elem<L>(S, stride, r, c);
                const int id = col_ids ? col_ids[c] : int(c);
                const bool after = (v < pv) || (v == pv && id > pi);
                const bool better = (v > bv) || (v == bv && id < bi);
                if (id != self && after && better) { bv = v; bi = id; }
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

}  // namespace

extern "C" {

int simrank_query_version(void) { return SIMRANK_QUERY_VERSION; }

const char* simrank_query_last_error(void) { return g_error.c_str(); }

int simrank_query_rows(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols, const int32_t* row_pos,
                       int64_t n_q, const int32_t* col_pos, int64_t n_out, double* out, int64_t ld_out, void* stream) {
    const int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    REQUIRE(n_q >= 0 && n_out >= 0 && ld_out >= n_out, "bad output shape %lld x %lld (ld %lld)", (long long)n_q,
                (long long)n_out, (long long)ld_out);
    REQUIRE(col_pos || n_out <= n_cols, "n_out %lld exceeds the block's %lld columns and there is no column map",
                (long long)n_out, (long long)n_cols);
    if (n_q == 0 || n_out == 0) return SIMRANK_QUERY_OK;
    REQUIRE(row_pos && out, "row_pos or out is NULL");
    const int64_t chunks = (n_out + kRowsChunk - 1) / kRowsChunk;
    const int64_t blocks = ((n_q + 7) / 8) * 8 * chunks;
    REQUIRE(blocks < (int64_t(1) << 31), "%lld x %lld values are too many for one call: cut the query rows into bands",
                (long long)n_q, (long long)n_out);
    hipStream_t st = as_stream(stream);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL(query_rows_kernel<L>, dim3((unsigned)blocks), dim3(kRowsThreads), 0, st, S, stride, n_rows,
                           n_cols, row_pos, n_q, col_pos, n_out, chunks, out, ld_out);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_QUERY_OK;
}

int simrank_query_pairs(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols, const int32_t* a_pos,
                        const int32_t* b_pos, int64_t n_pairs, double* out, void* stream) {
    const int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    REQUIRE(n_pairs >= 0 && n_pairs < (int64_t(1) << 38), "bad number of pairs %lld", (long long)n_pairs);
    if (n_pairs == 0) return SIMRANK_QUERY_OK;
    REQUIRE(a_pos && b_pos && out, "a_pos, b_pos or out is NULL");
    hipStream_t st = as_stream(stream);
    const unsigned grid = (unsigned)((n_pairs + 255) / 256);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL(query_pairs_kernel<L>, dim3(grid), dim3(256), 0, st, S, stride, n_rows, n_cols, a_pos, b_pos,
                           n_pairs, out);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_QUERY_OK;
}

int simrank_query_topk(const void* S, int32_t layout, int64_t stride, int64_t n_rows, int64_t n_cols, const int32_t* row_pos,
                       const int32_t* row_ids, int64_t n_q, const int32_t* col_ids, int32_t k, int32_t* idx_out,
                       double* val_out, void* stream) {
    const int rc = check_block(S, layout, stride, n_rows, n_cols);
    if (rc) return rc;
    REQUIRE(k >= 1 && k <= 1024, "k must be in [1, 1024] (got %d)", (int)k);
    REQUIRE(n_q >= 0 && n_q < (int64_t(1) << 31), "bad number of query rows %lld", (long long)n_q);
    if (n_q == 0) return SIMRANK_QUERY_OK;
    REQUIRE(row_pos && row_ids && idx_out && val_out, "row_pos, row_ids, idx_out or val_out is NULL");
    hipStream_t st = as_stream(stream);
    const unsigned grid = (unsigned)std::min<int64_t>((n_q + 3) / 4, int64_t(1) << 16);
    with_layout(layout, [&](auto L) {
        hipLaunchKernelGGL(query_topk_kernel<L>, dim3(grid), dim3(256), 0, st, S, stride, n_rows, n_cols, row_pos, row_ids,
                           n_q, col_ids, (int)k, idx_out, val_out);
    });
    HIP_CHECK(hipGetLastError());
    return SIMRANK_QUERY_OK;
}

int simrank_query_merge_topk(int32_t n_pieces, const int32_t* const* ids, const double* const* vals, const int32_t* ks,
                             int64_t n_q, int32_t k, int32_t* idx_out, double* val_out) {
    REQUIRE(n_pieces >= 0 && n_q >= 0 && k >= 1, "bad merge arguments");
    REQUIRE(n_q == 0 || (idx_out && val_out), "idx_out or val_out is NULL");
    for (int32_t p = 0; p < n_pieces; ++p)
        REQUIRE(ks && ks[p] >= 0 && (n_q == 0 || ks[p] == 0 || (ids && vals && ids[p] && vals[p])), "bad piece %d", (int)p);
    std::vector<std::pair<double, int32_t>> row;
    for (int64_t q = 0; q < n_q; ++q) {
        row.clear();
        for (int32_t p = 0; p < n_pieces; ++p)
            for (int32_t j = 0; j < ks[p]; ++j) {
                const int32_t id = ids[p][q * ks[p] + j];
                if (id >= 0) row.emplace_back(vals[p][q * ks[p] + j], id);
            }
        const size_t take = std::min<size_t>(size_t(k), row.size());
        std::partial_sort(row.begin(), row.begin() + take, row.end(),
                          [](const std::pair<double, int32_t>& a, const std::pair<double, int32_t>& b) {
                              return a.first > b.first || (a.first == b.first && a.second < b.second);
                          });
        for (int32_t j = 0; j < k; ++j) {
            idx_out[q * k + j] = size_t(j) < take ? row[j].second : -1;
            val_out[q * k + j] = size_t(j) < take ? row[j].first : 0.0;
        }
    }
    return SIMRANK_QUERY_OK;
}

}  // extern "C"
