// A kept model as one matrix in the caller's order (include/simrank_model.h, libsimrank_model.so): simrank_model_pack
// copies a block of an iterate, in the layout its plan stores it, into a block the caller owns, rows and columns
// permuted into the caller's order, optionally narrowed from f32 to the fp16-held form.
//
//     pack    dst[r][col_dst[i]] = src[row_map[r]][col_src[i]].  Shaped by its stores, as query_rows_kernel is: a
//             workgroup writes 256 x 16 bytes of consecutive entries of ONE destination row (1024 floats, 2048 halves or
//             512 doubles; one 16-byte store per lane where the destination columns are 0, 1, ... and its rows are
//             16-byte aligned) and GATHERS their sources from one source row: the column map scatters them over the row's
//             panel segments, but a whole source row is a small part of one XCD's L2, and all workgroups of a destination
//             row carry the same blockIdx % 8, so each segment comes from HBM once.  Every thread has 16 bytes' worth of
//             independent gathers in flight.  Element offsets are 64-bit (N^2 passes 2^31 at N = 46341); the rows are cut
//             into bands so that a launch stays below 2^32 work-items.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "simrank_model.h"

#define COMPANION_ERR_INVALID SIMRANK_MODEL_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_MODEL_ERR_HIP
#include "companion.h"

namespace {

COMPANION_SAME_LAYOUT(SIMRANK_MODEL_, PANEL_F32);
COMPANION_SAME_LAYOUT(SIMRANK_MODEL_, ROWMAJOR_F32);
COMPANION_SAME_LAYOUT(SIMRANK_MODEL_, PANEL_F16);
COMPANION_SAME_LAYOUT(SIMRANK_MODEL_, ROWMAJOR_F64);

constexpr int kThreads = 256;
constexpr int64_t kMaxBlocks = int64_t(1) << 23;          // x 256 threads = 2^31 work-items per launch

// Block b of a band: label x = b % 8 (the blocks that share an XCD), slot s = b / 8; the slots of a label walk the
// chunks of the band's rows 8 * (s / chunks) + x, so that every chunk of a destination row runs under the same label.
template <int SL, int DL>
__global__ __launch_bounds__(kThreads) void pack_kernel(const void* __restrict__ src, int64_t src_stride, int64_t src_rows,
                                                        int64_t src_cols, const int32_t* __restrict__ row_map,
                                                        const int32_t* __restrict__ col_dst,
                                                        const int32_t* __restrict__ col_src, int64_t n_list, int64_t chunks,
                                                        void* __restrict__ dst, int64_t dst_stride, int64_t row0,
                                                        int64_t band_rows, int64_t dst_cols, int vec,
                                                        unsigned long long* __restrict__ overflow) {
    using S = typename Stored<SL>::type;
    using D = typename Stored<DL>::type;
    constexpr int V = 16 / int(sizeof(D));
    constexpr bool kConvert = !(sizeof(S) == sizeof(D));
    const int64_t b = blockIdx.x;
    const int64_t slot = b >> 3;
    const int64_t rr = ((slot / chunks) << 3) + (b & 7);
    if (rr >= band_rows) return;                                  // (uniform over the workgroup)
    const int64_t r = row0 + rr;
    const int64_t sr = row_map ? int64_t(row_map[r]) : r;
    const bool row_ok = sr >= 0 && sr < src_rows;
    const int64_t i0 = ((slot % chunks) * kThreads + threadIdx.x) * V;
    const S* s = static_cast<const S*>(src);
    D* d = static_cast<D*>(dst);
    D v[V];
    bool ok[V];
    bool all = true;
    unsigned bad = 0;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const int64_t i = i0 + e;
        ok[e] = false;
        if (i < n_list && row_ok) {
            const int64_t sc = col_src ? int64_t(col_src[i]) : i;
            if (sc >= 0 && sc < src_cols) {
                const S x = s[offset_of<SL>(src_stride, sr, sc)];
                if constexpr (kConvert) {
                    // (a source of -0.0 came out of the conversion as +0.0 on the device: the sign of the stored value
                    // is the source's, whatever it rounds to)
                    const unsigned short h = __half_as_ushort(__float2half_rn(x * 16384.0f));
                    v[e] = __ushort_as_half((unsigned short)(h | ((__float_as_uint(x) >> 16) & 0x8000u)));
                    bad += (__half_as_ushort(v[e]) & 0x7c00u) == 0x7c00u;
                } else {
                    v[e] = x;
                }
                ok[e] = true;
            }
        }
        all = all && ok[e];
    }
    if (vec && all) {
        // (col_dst is NULL: the V entries are the destination columns i0 .. i0 + V - 1 < n_list <= dst_cols, i0 a
        // multiple of V, so they lie in one panel row or one aligned piece of a row-major row)
        uint4 u;
        __builtin_memcpy(&u, v, 16);
        *reinterpret_cast<uint4*>(d + offset_of<DL>(dst_stride, r, i0)) = u;
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (!ok[e]) continue;
            const int64_t i = i0 + e;
            const int64_t dc = col_dst ? int64_t(col_dst[i]) : i;
            if (dc >= 0 && dc < dst_cols) d[offset_of<DL>(dst_stride, r, dc)] = v[e];
        }
    }
    if constexpr (kConvert) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
        if ((threadIdx.x & 63) == 0 && bad) atomicAdd(overflow, (unsigned long long)bad);
    }
}

template <int SL, int DL>
int launch(const void* src, int64_t src_stride, int64_t src_rows, int64_t src_cols, const int32_t* row_map,
           const int32_t* col_dst, const int32_t* col_src, int64_t n_list, void* dst, int64_t dst_stride, int64_t dst_rows,
           int64_t dst_cols, int64_t* overflow, hipStream_t st) {
    using D = typename Stored<DL>::type;
    constexpr int V = 16 / int(sizeof(D));
    constexpr bool panels = DL == PANEL_F32 || DL == PANEL_F16;
    const int vec = !col_dst && (panels || dst_stride % V == 0);
    const int64_t chunks = (n_list + int64_t(kThreads) * V - 1) / (int64_t(kThreads) * V);
    const int64_t band = std::max<int64_t>(8, (kMaxBlocks / chunks) & ~int64_t(7));       // rows of one launch
    for (int64_t row0 = 0; row0 < dst_rows; row0 += band) {
        const int64_t m = std::min(band, dst_rows - row0);
        const int64_t blocks = ((m + 7) / 8) * 8 * chunks;        // <= max(8 * chunks, 2^23): below 2^32 work-items
        hipLaunchKernelGGL((pack_kernel<SL, DL>), dim3((unsigned)blocks), dim3(kThreads), 0, st, src, src_stride, src_rows,
                           src_cols, row_map, col_dst, col_src, n_list, chunks, dst, dst_stride, row0, m, dst_cols, vec,
                           reinterpret_cast<unsigned long long*>(overflow));
        HIP_CHECK(hipGetLastError());
    }
    return SIMRANK_MODEL_OK;
}

}  // namespace

extern "C" {

int simrank_model_version(void) { return SIMRANK_MODEL_VERSION; }

const char* simrank_model_last_error(void) { return g_error.c_str(); }

int simrank_model_pack(const void* src, int32_t src_layout, int64_t src_stride, int64_t src_rows, int64_t src_cols,
                       const int32_t* row_map, const int32_t* col_dst, const int32_t* col_src, int64_t n_list, void* dst,
                       int32_t dst_layout, int64_t dst_stride, int64_t dst_rows, int64_t dst_cols, int64_t* overflow,
                       void* stream) {
    int rc = check_block(src, src_layout, src_stride, src_rows, src_cols, "source");
    if (rc) return rc;
    rc = check_block(dst, dst_layout, dst_stride, dst_rows, dst_cols, "destination");
    if (rc) return rc;
    REQUIRE(n_list >= 0 && n_list < (int64_t(1) << 29), "bad number of columns %lld", (long long)n_list);
    REQUIRE(row_map || dst_rows <= src_rows, "%lld destination rows exceed the source's %lld and there is no row map",
            (long long)dst_rows, (long long)src_rows);
    REQUIRE(col_dst || n_list <= dst_cols, "%lld columns exceed the destination's %lld and there is no col_dst",
            (long long)n_list, (long long)dst_cols);
    REQUIRE(col_src || n_list <= src_cols, "%lld columns exceed the source's %lld and there is no col_src",
            (long long)n_list, (long long)src_cols);
    REQUIRE((reinterpret_cast<uintptr_t>(dst) & 15) == 0, "dst is not 16-byte aligned");
    const bool src_f32 = src_layout == SIMRANK_MODEL_PANEL_F32 || src_layout == SIMRANK_MODEL_ROWMAJOR_F32;
    const bool same = (src_f32 && dst_layout == SIMRANK_MODEL_ROWMAJOR_F32) ||
                      (src_layout == dst_layout && src_layout >= SIMRANK_MODEL_PANEL_F16);
    const bool converts = src_f32 && dst_layout == SIMRANK_MODEL_PANEL_F16;
    REQUIRE(same || converts, "no pack from layout %d to layout %d (f32 -> row-major f32 or fp16 panels, fp16 panels -> "
            "fp16 panels, float64 -> float64)", (int)src_layout, (int)dst_layout);
    REQUIRE(!converts || overflow, "overflow is NULL (a converting pack counts the values binary16 cannot hold)");
    if (dst_rows == 0 || n_list == 0) return SIMRANK_MODEL_OK;
    hipStream_t st = as_stream(stream);
#define PACK(SL, DL)                                                                                                       \
    return launch<SL, DL>(src, src_stride, src_rows, src_cols, row_map, col_dst, col_src, n_list, dst, dst_stride, dst_rows, \
                          dst_cols, overflow, st)
    if (dst_layout == SIMRANK_MODEL_ROWMAJOR_F32) {
        if (src_layout == SIMRANK_MODEL_PANEL_F32) PACK(PANEL_F32, ROWMAJOR_F32);
        PACK(ROWMAJOR_F32, ROWMAJOR_F32);
    }
    if (dst_layout == SIMRANK_MODEL_ROWMAJOR_F64) PACK(ROWMAJOR_F64, ROWMAJOR_F64);
    if (src_layout == SIMRANK_MODEL_PANEL_F16) PACK(PANEL_F16, PANEL_F16);
    if (src_layout == SIMRANK_MODEL_PANEL_F32) PACK(PANEL_F32, PANEL_F16);
    PACK(ROWMAJOR_F32, PANEL_F16);
#undef PACK
}

}  // extern "C"
