// Held-out ranks on a score band that stays on the device (include/simrank_rank.h, libsimrank_rank.so): the band's value
// at every target of a basket, and the number of candidates that precede each target in the total order of the top-k
// selection (value descending, id ascending).
//
//     gather  tgt_score[x] = band[q][tgt_col[x]] where the target's column is in this block; one wave per basket.
//     count   the geometry of sets_score_kernel: a workgroup owns one basket and 1024 consecutive band columns, a lane
//             owns 4 of them and keeps their values and ids in registers.  The basket's targets pass through local
//             memory in tiles of (score, id); for each staged target every lane forms its four predicates, the wave
//             counts each with one ballot, and one lane per wave adds the sum to the target's 32-bit word of local
//             memory.  After a tile every nonzero word becomes ONE 64-bit integer add to before[x] per workgroup; the
//             candidates of the row are counted the same way, once.  Integer adds: the result does not depend on the
//             schedule, and a model in several column blocks sums over its blocks by calling once per block.
//             A column past n_out is held as NaN, which is no candidate and precedes nothing.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "simrank_rank.h"

#define COMPANION_ERR_INVALID SIMRANK_RANK_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_RANK_ERR_HIP
#include "companion.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = 4;                              // band columns of one lane
constexpr int kChunk = kThreads * kPerThread;              // band columns of one workgroup
constexpr int kTile = SIMRANK_RANK_TILE;                   // targets staged together: one per lane of the workgroup
static_assert(kChunk == SIMRANK_RANK_CHUNK, "the header's chunk is the kernel's");
static_assert(kTile == kThreads, "a lane stages one target of a tile and flushes its word");

__global__ __launch_bounds__(256) void rank_gather_kernel(const double* __restrict__ band, int64_t ld_band, int64_t n_sets,
                                                          int64_t n_out, const int64_t* __restrict__ tgt_ptr,
                                                          const int32_t* __restrict__ tgt_col,
                                                          double* __restrict__ tgt_score) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t q = wave; q < n_sets; q += nwaves) {
        const double* row = band + q * ld_band;
        const int64_t x1 = tgt_ptr[q + 1];
        for (int64_t x = tgt_ptr[q] + lane; x < x1; x += 64) {
            const int64_t c = tgt_col[x];
            if (c >= 0 && c < n_out) tgt_score[x] = row[c];
        }
    }
}

// the lanes of the wave for which `p` holds (wave-uniform)
__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// VEC: the band's rows start on 16 bytes, so the 4 values of a full lane are two aligned vector loads
template <bool VEC>
__global__ __launch_bounds__(kThreads) void rank_count_kernel(const double* __restrict__ band, int64_t ld_band,
                                                              int64_t n_out, const int32_t* __restrict__ col_ids,
                                                              const int64_t* __restrict__ tgt_ptr,
                                                              const double* __restrict__ tgt_score,
                                                              const int32_t* __restrict__ tgt_id, int64_t chunks,
                                                              unsigned long long* __restrict__ before,
                                                              unsigned long long* __restrict__ candidates) {
    __shared__ double tile_s[kTile];
    __shared__ int32_t tile_t[kTile];
    __shared__ uint32_t tile_n[kTile];
    __shared__ uint32_t n_cand;
    const int64_t q = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int64_t x0 = tgt_ptr[q], x1 = tgt_ptr[q + 1];
    if (x0 >= x1) return;                                  // (workgroup-uniform: a basket without targets reads nothing)
    const int lane = threadIdx.x & 63;
    const int64_t j0 = chunk * kChunk + int64_t(threadIdx.x) * kPerThread;
    const double* row = band + q * ld_band;
    const double ninf = -__builtin_inf();

    // this lane's 4 values and ids; past n_out: NaN, which is no candidate and precedes nothing
    double v[kPerThread];
    int32_t id[kPerThread];
    if (VEC && j0 + kPerThread <= n_out) {
        const double2* p = reinterpret_cast<const double2*>(row + j0);
        const double2 a = p[0], b = p[1];
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    } else {
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) v[i] = j0 + i < n_out ? row[j0 + i] : __builtin_nan("");
    }
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) id[i] = (col_ids && j0 + i < n_out) ? col_ids[j0 + i] : int32_t(j0 + i);
    bool cand[kPerThread];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) cand[i] = v[i] > ninf;            // (false for NaN too)

    if (threadIdx.x == 0) n_cand = 0;
    for (int64_t t0 = x0; t0 < x1; t0 += kTile) {
        const int in_tile = x1 - t0 < kTile ? int(x1 - t0) : kTile;
        __syncthreads();                                   // (the previous tile's words are flushed; n_cand is zeroed)
        if ((int)threadIdx.x < in_tile) {
            tile_s[threadIdx.x] = tgt_score[t0 + threadIdx.x];
            tile_t[threadIdx.x] = tgt_id[t0 + threadIdx.x];
        }
        tile_n[threadIdx.x] = 0;
        __syncthreads();
        for (int k = 0; k < in_tile; ++k) {
            const double s = tile_s[k];
            const int32_t t = tile_t[k];
            uint32_t n = 0;
#pragma unroll
            for (int i = 0; i < kPerThread; ++i)
                n += wave_count(cand[i] && (v[i] > s || (v[i] == s && id[i] < t)));
            if (lane == 0 && n) atomicAdd(&tile_n[k], n);
        }
        __syncthreads();
        if ((int)threadIdx.x < in_tile && tile_n[threadIdx.x])
            atomicAdd(&before[t0 + threadIdx.x], (unsigned long long)tile_n[threadIdx.x]);
    }
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) n += wave_count(cand[i]);
    if (lane == 0 && n) atomicAdd(&n_cand, n);
    __syncthreads();
    if (threadIdx.x == 0 && n_cand) atomicAdd(&candidates[q], (unsigned long long)n_cand);
}

// ---- host --------------------------------------------------------------------------------------------------------------
int64_t grid_blocks(int64_t n_sets, int64_t n_out) {
    if (n_sets < 0 || n_out < 0 || n_sets >= (int64_t(1) << 31) || n_out >= (int64_t(1) << 31)) return -1;
    if (n_sets == 0 || n_out == 0) return 0;
    return n_sets * ((n_out + kChunk - 1) / kChunk);
}

int check_band(const double* band, int64_t ld_band, int64_t n_sets, int64_t n_out) {
    REQUIRE(n_sets >= 0 && n_sets < (int64_t(1) << 31) && n_out >= 0 && n_out < (int64_t(1) << 31) && ld_band >= n_out,
            "bad band shape %lld x %lld (ld %lld)", (long long)n_sets, (long long)n_out, (long long)ld_band);
    REQUIRE(band || n_sets == 0 || n_out == 0, "band is NULL");
    return 0;
}

}  // namespace

extern "C" {

int simrank_rank_version(void) { return SIMRANK_RANK_VERSION; }

const char* simrank_rank_last_error(void) { return g_error.c_str(); }

int64_t simrank_rank_blocks(int64_t n_sets, int64_t n_out) { return grid_blocks(n_sets, n_out); }

int simrank_rank_gather(const double* band, int64_t ld_band, int64_t n_sets, int64_t n_out, const int64_t* tgt_ptr,
                        const int32_t* tgt_col, double* tgt_score, void* stream) {
    const int rc = check_band(band, ld_band, n_sets, n_out);
    if (rc) return rc;
    if (n_sets == 0 || n_out == 0) return SIMRANK_RANK_OK;
    REQUIRE(tgt_ptr, "tgt_ptr is NULL");
    // (tgt_col and tgt_score may be NULL when no basket has a target: they are then never read)
    const unsigned grid = (unsigned)std::min<int64_t>((n_sets + kWaves - 1) / kWaves, int64_t(1) << 16);
    hipLaunchKernelGGL(rank_gather_kernel, dim3(grid), dim3(256), 0, as_stream(stream), band, ld_band, n_sets, n_out,
                       tgt_ptr, tgt_col, tgt_score);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_RANK_OK;
}

int simrank_rank_count(const double* band, int64_t ld_band, int64_t n_sets, int64_t n_out, const int32_t* col_ids,
                       const int64_t* tgt_ptr, const double* tgt_score, const int32_t* tgt_id, int64_t* before,
                       int64_t* candidates, void* stream) {
    const int rc = check_band(band, ld_band, n_sets, n_out);
    if (rc) return rc;
    const int64_t blocks = grid_blocks(n_sets, n_out);
    REQUIRE(blocks <= SIMRANK_RANK_MAX_BLOCKS, "%lld baskets x %lld columns are too many for one call (%lld workgroups): "
            "cut the baskets into bands", (long long)n_sets, (long long)n_out, (long long)blocks);
    if (blocks == 0) return SIMRANK_RANK_OK;
    REQUIRE(tgt_ptr && candidates, "tgt_ptr or candidates is NULL");
    // (tgt_score, tgt_id and before may be NULL when no basket has a target: they are then never touched)
    const int64_t chunks = (n_out + kChunk - 1) / kChunk;
    const bool vec = reinterpret_cast<uintptr_t>(band) % 16 == 0 && ld_band % 2 == 0;
    unsigned long long* b = reinterpret_cast<unsigned long long*>(before);
    unsigned long long* c = reinterpret_cast<unsigned long long*>(candidates);
    hipStream_t st = as_stream(stream);
    if (vec)
        hipLaunchKernelGGL(rank_count_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, band, ld_band, n_out,
                           col_ids, tgt_ptr, tgt_score, tgt_id, chunks, b, c);
    else
        hipLaunchKernelGGL(rank_count_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, band, ld_band, n_out,
                           col_ids, tgt_ptr, tgt_score, tgt_id, chunks, b, c);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_RANK_OK;
}

}  // extern "C"
