// The reference's float64 loop on one GPU (include/simrank_f64.h, libsimrank_f64.so): fit(storage_precision="f64").
//
// An update X' = C . W Y W^T (.* E) (blend) with W = diag(r) . P runs as two gather legs over 16 x 16 tiles of doubles
// (one 128-byte line per row and tile), 256 threads per tile, one output element per thread:
//     leg A   T = W Y: thread (i, c) sums Y[j][c] over j in P(i), times r_i; the tile goes out transposed through LDS
//             (T^T[c][i0 .. i0 + 15] is one line), so that leg B gathers rows of it.
//     leg B   O = W T^T = (W Y W^T)^T: thread (b, a) sums T^T[j][a] over j in P(b), times r_b.  Symmetric iterates: only
//             the tiles on or above the diagonal, the epilogue and the count fused, then a mirror pass copies the upper
//             triangle down.  Otherwise O is stored raw and a tiled in-place transpose pass applies the epilogue to
//             S'[r][c] = f(O[c][r]) (a workgroup owns a tile and its mirror image, so in place is safe).
// Tiles go panel-major (consecutive tiles share a 16-column panel of the gathered matrix, whose N x 128 bytes stay
// L2-resident) and are dealt to the eight XCDs in contiguous runs (workgroup w runs on XCD w % 8).  The gathers go
// in CSR order with one accumulator, so every element's sum has one fixed order: two runs give the same bits.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "simrank_f64.h"

#define COMPANION_ERR_INVALID SIMRANK_F64_ERR_INVALID
#define COMPANION_ERR_HIP SIMRANK_F64_ERR_HIP
#include "companion.h"

namespace {

constexpr int kTile = 16;
constexpr int kSlots = 1024;              // convergence counters, spread so that tiles seldom meet on one address

// row pitch in doubles: whole 128-byte lines, and never a large power of two (a panel's lines would share channels)
int64_t pitch(int64_t n) {
    int64_t ld = (std::max<int64_t>(n, 1) + kTile - 1) / kTile * kTile;
    if (ld >= 2048 && (ld & (ld - 1)) == 0) ld += kTile;
    return ld;
}

int64_t round8(int64_t x) { return (x + 7) / 8 * 8; }

unsigned tiles_grid(int64_t ntiles);

// The first tile of this workgroup: the grid is a multiple of 8 workgroups, XCD x = w % 8 takes the x-th contiguous
// run of it; a workgroup then steps by the grid (at most kMaxGrid workgroups: the grid's work-items must stay below
// 2^32, which N = 65536 would pass with one tile per workgroup).
__device__ inline int64_t xcd_tile() {
    const int64_t w = blockIdx.x;
    return (w & 7) * (int64_t(gridDim.x) >> 3) + (w >> 3);
}

constexpr int64_t kMaxGrid = int64_t(1) << 19;

struct Epi {
    double coef, lbd, eps;
    const uint8_t* counts;                // NULL: no evidence factor
    int64_t cld, cn;                      // cn = 1: one count for every pair (a 1 x 1 Evidence broadcast)
    const double* prior;                  // NULL: no prior
    int64_t ld;                           // pitch of the prior and the iterates
};

// SimRank.py:139 / :361 / :453 in the reference's evaluation order, then diag = 1 (no contraction into FMAs)
__device__ inline double epilogue(const Epi& e, double prod, int64_t r, int64_t c) {
#pragma clang fp contract(off)
    if (r == c) return 1.0;
    if (e.counts || e.prior) {
        double E = 1.0;
        if (e.counts) {
            const int cnt = e.cn == 1 ? e.counts[0] : e.counts[r * e.cld + c];
            E = 1.0 - ldexp(1.0, -cnt);
        }
        if (e.prior) return (1.0 - e.lbd) * E * e.coef * prod + e.lbd * e.prior[r * e.ld + c];
        return E * e.coef * prod;
    }
    return e.coef * prod;
}

__device__ inline void add_count(unsigned v, unsigned long long* slots) {
    __shared__ unsigned red[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned s = red[0] + red[1] + red[2] + red[3];
        if (s) atomicAdd(slots + (blockIdx.x & (kSlots - 1)), (unsigned long long)s);
    }
}

// sum of G[j * ldg + c] over j = col[p], p in [p0, p1), CSR order, four loads in flight
__device__ inline double gather(const int32_t* __restrict__ col, int p0, int p1, const double* __restrict__ G,
                                int64_t ldg, int64_t c) {
    double acc = 0.0;
    int p = p0;
    for (; p + 4 <= p1; p += 4) {
        const int64_t j0 = col[p], j1 = col[p + 1], j2 = col[p + 2], j3 = col[p + 3];
        const double v0 = G[j0 * ldg + c], v1 = G[j1 * ldg + c], v2 = G[j2 * ldg + c], v3 = G[j3 * ldg + c];
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
    }
    for (; p < p1; ++p) acc += G[int64_t(col[p]) * ldg + c];
    return acc;
}

// leg A: T^T[c][i] = r_i . sum_{j in P(i)} Y[j][c], i < n_w, c < n_y
__global__ __launch_bounds__(256) void leg_a_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                    const double* __restrict__ rs, const double* __restrict__ Y, int64_t ldy,
                                                    int64_t n_w, int64_t n_y, double* __restrict__ Tt, int64_t ldt,
                                                    int64_t nrb, int64_t ntiles) {
    __shared__ double tile[kTile][kTile + 1];
    const int t = threadIdx.x, rl = t >> 4, cl = t & 15;
    for (int64_t L = xcd_tile(); L < ntiles; L += gridDim.x) {
        const int64_t panel = L / nrb, rb = L % nrb;
        const int64_t i = rb * kTile + rl, c = panel * kTile + cl;
        double v = 0.0;
        if (i < n_w && c < n_y) {
            const double r = rs[i];
            if (r != 0.0) v = r * gather(col, rowptr[i], rowptr[i + 1], Y, ldy, c);
        }
        tile[rl][cl] = v;
        __syncthreads();
        const int64_t cc = panel * kTile + rl, ii = rb * kTile + cl;
        if (cc < n_y && ii < n_w) Tt[cc * ldt + ii] = tile[cl][rl];
        __syncthreads();
    }
}

// leg B: O[b][a] = r_b . sum_{j in P(b)} T^T[j][a].  SYM: tiles on or above the diagonal, elements a >= b, the epilogue
// and the count fused (an element off the diagonal counts twice: it stands for its mirror image too).  Otherwise raw O.
template <bool SYM>
__global__ __launch_bounds__(256) void leg_b_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                    const double* __restrict__ rs, const double* __restrict__ Tt,
                                                    int64_t ldt, int64_t n_w, Epi e, const double* __restrict__ Sold,
                                                    double* __restrict__ X, int64_t nrb, int64_t ntiles,
                                                    unsigned long long* slots) {
    const int t = threadIdx.x;
    unsigned changed = 0;
    for (int64_t L = xcd_tile(); L < ntiles; L += gridDim.x) {
        const int64_t panel = L / nrb, rb = L % nrb;
        if (SYM && panel < rb) continue;
        const int64_t b = rb * kTile + (t >> 4), a = panel * kTile + (t & 15);
        if (b < n_w && a < n_w && (!SYM || a >= b)) {
            const double r = rs[b];
            const double prod = r != 0.0 ? r * gather(col, rowptr[b], rowptr[b + 1], Tt, ldt, a) : 0.0;
            if (SYM) {
                const double v = epilogue(e, prod, b, a);
                if (fabs(v - Sold[b * e.ld + a]) > e.eps) changed += a == b ? 1 : 2;
                X[b * e.ld + a] = v;
            } else {
                X[b * e.ld + a] = prod;
            }
        }
    }
    if (SYM) add_count(changed, slots);
}

// full form: tile pair (I, J), I <= J, of the raw O in X: S'[r][c] = epilogue(O[c][r]) at both tiles, in place
__global__ __launch_bounds__(256) void transpose_epilogue_kernel(double* __restrict__ X, const double* __restrict__ Sold,
                                                                 int64_t n, Epi e, int64_t nb,
                                                                 unsigned long long* slots) {
    __shared__ double t0[kTile][kTile + 1], t1[kTile][kTile + 1];
    const int t = threadIdx.x, rl = t >> 4, cl = t & 15;
    unsigned changed = 0;
    for (int64_t L = blockIdx.x; L < nb * nb; L += gridDim.x) {
        const int64_t I = L / nb, J = L % nb;
        if (I > J) continue;
        const int64_t r0 = I * kTile + rl, c0 = J * kTile + cl;      // tile (I, J)
        const int64_t r1 = J * kTile + rl, c1 = I * kTile + cl;      // tile (J, I)
        t0[rl][cl] = (r0 < n && c0 < n) ? X[r0 * e.ld + c0] : 0.0;
        t1[rl][cl] = (r1 < n && c1 < n) ? X[r1 * e.ld + c1] : 0.0;
        __syncthreads();
        if (r0 < n && c0 < n) {
            const double v = epilogue(e, t1[cl][rl], r0, c0);
            changed += fabs(v - Sold[r0 * e.ld + c0]) > e.eps;
            X[r0 * e.ld + c0] = v;
        }
        if (I != J && r1 < n && c1 < n) {
            const double v = epilogue(e, t0[cl][rl], r1, c1);
            changed += fabs(v - Sold[r1 * e.ld + c1]) > e.eps;
            X[r1 * e.ld + c1] = v;
        }
        __syncthreads();
    }
    add_count(changed, slots);
}

// symmetric form: X[r][c] = X[c][r] for r > c, from the upper tile (I, J), I <= J, into the lower (J, I)
__global__ __launch_bounds__(256) void mirror_kernel(double* __restrict__ X, int64_t ld, int64_t n, int64_t nb) {
    __shared__ double tile[kTile][kTile + 1];
    const int t = threadIdx.x, rl = t >> 4, cl = t & 15;
    for (int64_t L = blockIdx.x; L < nb * nb; L += gridDim.x) {
        const int64_t I = L / nb, J = L % nb;
        if (I > J) continue;
        const int64_t r0 = I * kTile + rl, c0 = J * kTile + cl;
        tile[rl][cl] = (r0 < n && c0 < n) ? X[r0 * ld + c0] : 0.0;
        __syncthreads();
        const int64_t r1 = J * kTile + rl, c1 = I * kTile + cl;
        if (r1 < n && c1 < n && (I != J || rl > cl)) X[r1 * ld + c1] = tile[cl][rl];
        __syncthreads();
    }
}

__global__ void identity_kernel(double* X, int64_t ld, int64_t n) {
    const int64_t total = n * ld;
    for (int64_t q = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; q < total; q += int64_t(gridDim.x) * blockDim.x) {
        const int64_t r = q / ld, c = q % ld;
        X[q] = r == c ? 1.0 : 0.0;
    }
}

// ---- hand-backs ----

// top-k, one wave per row: K best of the lane's columns in registers (value descending, id ascending), then the wave
// takes the best head k times (k <= K)
template <int K>
__global__ __launch_bounds__(256) void topk_onepass_kernel(const double* __restrict__ S, int64_t ld, int64_t n, int k,
                                                           int exclude_diag, int32_t* idx_out, double* val_out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t a = wave; a < n; a += nwaves) {
        const int64_t skip = exclude_diag ? a : -1;
        double tv[K];
        int ti[K];
#pragma unroll
        for (int i = 0; i < K; ++i) { tv[i] = -__builtin_inf(); ti[i] = 0x7fffffff; }
        const double* row = S + a * ld;
        for (int64_t c = lane; c < n; c += 64) {
            double v = row[c];
            int id = int(c);
            if (c != skip && ((v > tv[K - 1]) || (v == tv[K - 1] && id < ti[K - 1]))) {
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const bool better = (v > tv[i]) || (v == tv[i] && id < ti[i]);
                    const double nv = better ? tv[i] : v;
                    const int ni = better ? ti[i] : id;
                    tv[i] = better ? v : tv[i];
                    ti[i] = better ? id : ti[i];
                    v = nv;
                    id = ni;
                }
            }
        }
        for (int j = 0; j < k; ++j) {
            double bv = tv[0];
            int bi = ti[0];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                if ((ov > bv) || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            const bool found = bi != 0x7fffffff;
            if (lane == 0) {
                idx_out[a * k + j] = found ? bi : -1;
                val_out[a * k + j] = found ? bv : 0.0;
            }
            if (found && ti[0] == bi) {          // ids are distinct: exactly one lane owns the pick; it pops its head
#pragma unroll
                for (int i = 0; i + 1 < K; ++i) { tv[i] = tv[i + 1]; ti[i] = ti[i + 1]; }
                tv[K - 1] = -__builtin_inf();
                ti[K - 1] = 0x7fffffff;
            }
        }
    }
}

// any k: k rounds of "the largest element after the previous pick" in the same total order
__global__ __launch_bounds__(256) void topk_rounds_kernel(const double* __restrict__ S, int64_t ld, int64_t n, int k,
                                                          int exclude_diag, int32_t* idx_out, double* val_out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t a = wave; a < n; a += nwaves) {
        const int64_t skip = exclude_diag ? a : -1;
        double pv = __builtin_inf();
        int pi = -1;
        for (int j = 0; j < k; ++j) {
            double bv = -__builtin_inf();
            int bi = 0x7fffffff;
            for (int64_t c = lane; c < n; c += 64) {
                const double v = S[a * ld + c];
                const int id = int(c);
                const bool after = (v < pv) || (v == pv && id > pi);
                const bool better = (v > bv) || (v == bv && id < bi);
                if (c != skip && after && better) { bv = v; bi = id; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                if ((ov > bv) || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            const bool found = bi != 0x7fffffff;
            if (lane == 0) {
                idx_out[a * k + j] = found ? bi : -1;
                val_out[a * k + j] = found ? bv : 0.0;
            }
            if (!found) {
                if (lane == 0)
                    for (int jj = j + 1; jj < k; ++jj) { idx_out[a * k + jj] = -1; val_out[a * k + jj] = 0.0; }
                break;
            }
            pv = bv;
            pi = bi;
        }
    }
}

// threshold selection, one wave per row, 64 columns per step: COUNT writes counts[r]; EMIT writes hit j of row r at
// offsets[r] + j (rank from the ballot's prefix count), never at or past offsets[r + 1] nor capacity
template <bool EMIT>
__global__ __launch_bounds__(256) void above_kernel(const double* __restrict__ S, int64_t ld, int64_t n, double t,
                                                    int32_t* counts, const int64_t* __restrict__ offsets,
                                                    int64_t capacity, int32_t* ids, double* vals) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    for (int64_t r = wave; r < n; r += nwaves) {
        const double* row = S + r * ld;
        int64_t pos = EMIT ? offsets[r] : 0;
        const int64_t end = EMIT ? (offsets[r + 1] < capacity ? offsets[r + 1] : capacity) : 0;
        for (int64_t c0 = 0; c0 < n; c0 += 64) {
            const int64_t c = c0 + lane;
            const double v = c < n ? row[c] : 0.0;
            const bool hit = c < n && c != r && v >= t;
            const unsigned long long m = __ballot(hit);
            if (EMIT && hit) {
                const int64_t q = pos + __popcll(m & below);
                if (q < end) {
                    ids[q] = int32_t(c);
                    vals[q] = v;
                }
            }
            pos += __popcll(m);
        }
        if (!EMIT && lane == 0) counts[r] = int32_t(pos);
    }
}

struct Side {
    int64_t n = 0, m = 0, nnz = 0, ld = 0;
    int32_t* rowptr = nullptr;
    int32_t* col = nullptr;
    double* rs = nullptr;
    double coef = 0.8, lbd = 0.0;
    const uint8_t* counts = nullptr;
    int64_t cld = 0, cn = 0;
    double* prior = nullptr;
    double* S[2] = {nullptr, nullptr};
    int cur = 0;
};

int64_t side_bytes(const simrank_f64_side& s) {
    const int64_t ld = pitch(s.n_rows);
    const int64_t mat = s.n_rows * ld * 8;
    return 2 * mat + (s.prior ? mat : 0) + 4 * (s.n_rows + 1) + 4 * std::max<int64_t>(s.nnz, 1) + 8 * s.n_rows;
}

int64_t t_elems(const simrank_f64_side* sides, int32_t n_sides) {
    int64_t t = 0;
    for (int32_t u = 0; u < n_sides; ++u) t = std::max(t, sides[u].n_cols * pitch(sides[u].n_rows));
    return t;
}

int check_sides(const simrank_f64_side* sides, int32_t n_sides) {
    REQUIRE(sides, "sides is NULL");
    REQUIRE(n_sides == 1 || n_sides == 2, "n_sides must be 1 or 2 (got %d)", (int)n_sides);
    for (int32_t u = 0; u < n_sides; ++u) {
        const simrank_f64_side& s = sides[u];
        REQUIRE(s.n_rows > 0 && s.n_cols > 0 && s.n_rows < (int64_t(1) << 31) && s.n_cols < (int64_t(1) << 31),
                    "side %d: bad shape %lld x %lld", (int)u, (long long)s.n_rows, (long long)s.n_cols);
        REQUIRE(s.nnz >= 0 && s.nnz < (int64_t(1) << 31), "side %d: bad nnz %lld", (int)u, (long long)s.nnz);
        REQUIRE(s.rowptr && s.rowscale && (s.col || s.nnz == 0), "side %d: rowptr, col or rowscale is NULL", (int)u);
        REQUIRE(s.rowptr[0] == 0 && s.rowptr[s.n_rows] == s.nnz, "side %d: rowptr does not run from 0 to nnz", (int)u);
        for (int64_t r = 0; r < s.n_rows; ++r)
            REQUIRE(s.rowptr[r + 1] >= s.rowptr[r], "side %d: rowptr decreases at row %lld", (int)u, (long long)r);
        for (int64_t p = 0; p < s.nnz; ++p)
            REQUIRE(s.col[p] >= 0 && s.col[p] < s.n_cols, "side %d: column %d out of range at %lld", (int)u,
                        (int)s.col[p], (long long)p);
        REQUIRE(!s.counts || ((s.counts_n == s.n_rows || s.counts_n == 1) && s.counts_ld >= s.counts_n),
                    "side %d: counts must be n x n or 1 x 1 with ld >= n", (int)u);
    }
    if (n_sides == 1)
        REQUIRE(sides[0].n_rows == sides[0].n_cols, "one side needs a square pattern");
    else
        REQUIRE(sides[1].n_rows == sides[0].n_cols && sides[1].n_cols == sides[0].n_rows &&
                        sides[1].nnz == sides[0].nnz, "side 1's pattern must be the transpose of side 0's");
    return SIMRANK_F64_OK;
}

}  // namespace

struct simrank_f64_plan {
    Side s[2];
    int32_t ns = 1;
    int32_t sym = 1;
    hipStream_t stream = nullptr;
    double* T = nullptr;
    unsigned long long* slots = nullptr;     // [2][kSlots]
    bool released = false;
    // selection state of the last _count_above
    int32_t sel_side = -1;
    double sel_t = 0.0;
    int64_t* sel_off = nullptr;
    int64_t sel_n = 0;
    // timing
    bool timing = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[3] = {0, 0, 0};
    int32_t steps = 0;
};

namespace {

void free_plan(simrank_f64_plan* p) {
    for (auto& s : p->s) {
        (void)hipFree(s.rowptr);
        (void)hipFree(s.col);
        (void)hipFree(s.rs);
        (void)hipFree(s.prior);
        (void)hipFree(s.S[0]);
        (void)hipFree(s.S[1]);
        s.rowptr = s.col = nullptr;
        s.rs = s.prior = s.S[0] = s.S[1] = nullptr;
    }
    (void)hipFree(p->T);
    (void)hipFree(p->slots);
    (void)hipFree(p->sel_off);
    p->T = nullptr;
    p->slots = nullptr;
    p->sel_off = nullptr;
    p->sel_side = -1;
}

template <class T>
int dmalloc(T** ptr, int64_t count) {
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(ptr), size_t(std::max<int64_t>(count, 1)) * sizeof(T)));
    return SIMRANK_F64_OK;
}

unsigned tiles_grid(int64_t ntiles) { return (unsigned)std::min(round8(ntiles), kMaxGrid); }

int launch_identity(double* X, int64_t ld, int64_t n, hipStream_t st) {
    const int64_t total = n * ld;
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(identity_kernel, dim3(grid), dim3(256), 0, st, X, ld, n);
    HIP_CHECK(hipGetLastError());
    return SIMRANK_F64_OK;
}

// side u's update: reads Y (side 1 - u's matrix with two sides, its own with one), writes S[cur ^ 1] and the count
int update(simrank_f64_plan* p, int u, double eps) {
    Side& s = p->s[u];
    const Side& y = p->s[p->ns == 2 ? 1 - u : u];
    const double* Y = y.S[y.cur];
    const double* Sold = s.S[s.cur];
    double* X = s.S[s.cur ^ 1];
    const int64_t n_w = s.n, n_y = s.m, ldt = pitch(n_w);
    const int64_t nrb = (n_w + kTile - 1) / kTile, npa = (n_y + kTile - 1) / kTile;
    unsigned long long* slots = p->slots + u * kSlots;
    const bool t = p->timing;
    if (t) HIP_CHECK(hipEventRecord(p->ev[0], p->stream));
    const int64_t ta = nrb * npa;
    hipLaunchKernelGGL(leg_a_kernel, dim3(tiles_grid(ta)), dim3(256), 0, p->stream, s.rowptr, s.col, s.rs, Y, y.ld,
                       n_w, n_y, p->T, ldt, nrb, ta);
    HIP_CHECK(hipGetLastError());
    if (t) HIP_CHECK(hipEventRecord(p->ev[1], p->stream));
    Epi e{s.coef, s.lbd, eps, s.counts, s.cld, s.cn, s.prior, s.ld};
    const int64_t tb = nrb * nrb;
    if (p->sym)
        hipLaunchKernelGGL(leg_b_kernel<true>, dim3(tiles_grid(tb)), dim3(256), 0, p->stream, s.rowptr, s.col, s.rs,
                           p->T, ldt, n_w, e, Sold, X, nrb, tb, slots);
    else
        hipLaunchKernelGGL(leg_b_kernel<false>, dim3(tiles_grid(tb)), dim3(256), 0, p->stream, s.rowptr, s.col,
                           s.rs, p->T, ldt, n_w, e, Sold, X, nrb, tb, slots);
    HIP_CHECK(hipGetLastError());
    if (t) HIP_CHECK(hipEventRecord(p->ev[2], p->stream));
    if (p->sym)
        hipLaunchKernelGGL(mirror_kernel, dim3(tiles_grid(tb)), dim3(256), 0, p->stream, X, s.ld, n_w, nrb);
    else
        hipLaunchKernelGGL(transpose_epilogue_kernel, dim3(tiles_grid(tb)), dim3(256), 0, p->stream, X, Sold, n_w, e, nrb,
                           slots);
    HIP_CHECK(hipGetLastError());
    if (t) HIP_CHECK(hipEventRecord(p->ev[3], p->stream));
    s.cur ^= 1;
    if (t) {
        HIP_CHECK(hipEventSynchronize(p->ev[3]));
        for (int q = 0; q < 3; ++q) {
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, p->ev[q], p->ev[q + 1]));
            p->ms[q] += ms;
        }
    }
    return SIMRANK_F64_OK;
}

int side_ok(simrank_f64_plan* p, int32_t side) {
    REQUIRE(p, "plan is NULL");
    REQUIRE(side >= 0 && side < p->ns, "side %d out of range (the plan has %d)", (int)side, (int)p->ns);
    REQUIRE(!p->released, "the plan's matrices were released (simrank_f64_plan_trim)");
    return SIMRANK_F64_OK;
}

int waves_grid(int64_t rows) { return (int)std::min<int64_t>((rows + 3) / 4, 256 * 8); }

}  // namespace

extern "C" {

int simrank_f64_version(void) { return SIMRANK_F64_VERSION; }

const char* simrank_f64_last_error(void) { return g_error.c_str(); }

int simrank_f64_plan_bytes(const simrank_f64_side* sides, int32_t n_sides, int64_t* bytes) {
    REQUIRE(bytes, "bytes is NULL");
    const int rc = check_sides(sides, n_sides);
    if (rc) return rc;
    int64_t b = 8 * t_elems(sides, n_sides) + 8 * 2 * kSlots;
    for (int32_t u = 0; u < n_sides; ++u) b += side_bytes(sides[u]);
    *bytes = b;
    return SIMRANK_F64_OK;
}

int simrank_f64_mem_info(int64_t* free_bytes, int64_t* total_bytes) {
    REQUIRE(free_bytes && total_bytes, "NULL argument");
    size_t f = 0, t = 0;
    HIP_CHECK(hipMemGetInfo(&f, &t));
    *free_bytes = (int64_t)f;
    *total_bytes = (int64_t)t;
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_create(const simrank_f64_side* sides, int32_t n_sides, const simrank_f64_options* options,
                            void* stream, simrank_f64_plan** out) {
    REQUIRE(out, "out is NULL");
    *out = nullptr;
    int64_t need = 0;
    int rc = simrank_f64_plan_bytes(sides, n_sides, &need);
    if (rc) return rc;
    size_t f = 0, tot = 0;
    HIP_CHECK(hipMemGetInfo(&f, &tot));
    if (need > (int64_t)f) {
        set_error("storage_precision='f64' needs %.2f GiB of device memory for its matrices; %.2f GiB of %.2f GiB are free",
                  need / 1073741824.0, f / 1073741824.0, tot / 1073741824.0);
        return SIMRANK_F64_ERR_MEMORY;
    }
    auto* p = new simrank_f64_plan();
    p->ns = n_sides;
    p->sym = options ? (options->symmetric != 0) : 1;
    p->stream = as_stream(stream);
    auto fail = [&](int code) {
        free_plan(p);
        delete p;
        return code;
    };
    for (int32_t u = 0; u < n_sides; ++u) {
        const simrank_f64_side& d = sides[u];
        Side& s = p->s[u];
        s.n = d.n_rows;
        s.m = d.n_cols;
        s.nnz = d.nnz;
        s.ld = pitch(s.n);
        s.coef = d.coef;
        s.lbd = d.lbd;
        s.counts = d.counts;
        s.cld = d.counts_ld;
        s.cn = d.counts_n;
        if ((rc = dmalloc(&s.rowptr, s.n + 1)) || (rc = dmalloc(&s.col, s.nnz)) || (rc = dmalloc(&s.rs, s.n)) ||
            (rc = dmalloc(&s.S[0], s.n * s.ld)) || (rc = dmalloc(&s.S[1], s.n * s.ld)) ||
            (d.prior && (rc = dmalloc(&s.prior, s.n * s.ld))))
            return fail(rc);
        hipError_t e = hipMemcpyAsync(s.rowptr, d.rowptr, size_t(s.n + 1) * 4, hipMemcpyHostToDevice, p->stream);
        if (e == hipSuccess && s.nnz)
            e = hipMemcpyAsync(s.col, d.col, size_t(s.nnz) * 4, hipMemcpyHostToDevice, p->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(s.rs, d.rowscale, size_t(s.n) * 8, hipMemcpyHostToDevice, p->stream);
        if (e == hipSuccess && d.prior)
            e = hipMemcpy2DAsync(s.prior, size_t(s.ld) * 8, d.prior, size_t(s.n) * 8, size_t(s.n) * 8, size_t(s.n),
                                 hipMemcpyHostToDevice, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);      // (the host arrays are the caller's)
        if (e != hipSuccess) {
            set_error("simrank_f64_plan_create: upload failed: %s", hipGetErrorString(e));
            (void)hipGetLastError();
            return fail(SIMRANK_F64_ERR_HIP);
        }
    }
    if ((rc = dmalloc(&p->T, t_elems(sides, n_sides))) || (rc = dmalloc(&p->slots, 2 * kSlots))) return fail(rc);
    for (auto& ev : p->ev) {
        if (hipEventCreate(&ev) != hipSuccess) {
            set_error("simrank_f64_plan_create: hipEventCreate failed");
            return fail(SIMRANK_F64_ERR_HIP);
        }
    }
    *out = p;
    rc = simrank_f64_plan_reset(p);
    if (rc) {
        simrank_f64_plan_destroy(p);
        *out = nullptr;
    }
    return rc;
}

int simrank_f64_plan_destroy(simrank_f64_plan* p) {
    if (!p) return SIMRANK_F64_OK;
    (void)hipStreamSynchronize(p->stream);
    free_plan(p);
    for (auto& ev : p->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete p;
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_reset(simrank_f64_plan* p) {
    REQUIRE(p, "plan is NULL");
    REQUIRE(!p->released, "the plan's matrices were released (simrank_f64_plan_trim)");
    for (int32_t u = 0; u < p->ns; ++u) {
        Side& s = p->s[u];
        s.cur = 0;
        const int rc = launch_identity(s.S[0], s.ld, s.n, p->stream);
        if (rc) return rc;
    }
    HIP_CHECK(hipStreamSynchronize(p->stream));
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_step(simrank_f64_plan* p, double eps, int64_t* changed) {
    REQUIRE(p && changed, "NULL argument");
    REQUIRE(!p->released, "the plan's matrices were released (simrank_f64_plan_trim)");
    HIP_CHECK(hipMemsetAsync(p->slots, 0, sizeof(unsigned long long) * 2 * kSlots, p->stream));
    for (int32_t u = 0; u < p->ns; ++u) {
        const int rc = update(p, u, eps);
        if (rc) return rc;
    }
    std::vector<unsigned long long> h(2 * kSlots);
    HIP_CHECK(hipMemcpyAsync(h.data(), p->slots, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost, p->stream));
    HIP_CHECK(hipStreamSynchronize(p->stream));
    for (int32_t u = 0; u < p->ns; ++u) {
        unsigned long long c = 0;
        for (int q = 0; q < kSlots; ++q) c += h[u * kSlots + q];
        changed[u] = (int64_t)c;
    }
    if (p->timing) ++p->steps;
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_set_timing(simrank_f64_plan* p, int32_t on) {
    REQUIRE(p, "plan is NULL");
    p->timing = on != 0;
    p->ms[0] = p->ms[1] = p->ms[2] = 0;
    p->steps = 0;
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_leg_times(simrank_f64_plan* p, double* ms, int32_t* steps) {
    REQUIRE(p && ms && steps, "NULL argument");
    for (int q = 0; q < 3; ++q) ms[q] = p->ms[q];
    *steps = p->steps;
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_result(simrank_f64_plan* p, int32_t side, double* dst, int64_t ld) {
    int rc = side_ok(p, side);
    if (rc) return rc;
    const Side& s = p->s[side];
    REQUIRE(dst && ld >= s.n, "bad result arguments (dst NULL or ld < %lld)", (long long)s.n);
    HIP_CHECK(hipMemcpy2DAsync(dst, size_t(ld) * 8, s.S[s.cur], size_t(s.ld) * 8, size_t(s.n) * 8, size_t(s.n),
                             hipMemcpyDeviceToHost, p->stream));
    HIP_CHECK(hipStreamSynchronize(p->stream));
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_topk(simrank_f64_plan* p, int32_t side, int32_t k, int32_t exclude_diag, int32_t* idx_host,
                          double* val_host) {
    int rc = side_ok(p, side);
    if (rc) return rc;
    const Side& s = p->s[side];
    REQUIRE(idx_host && val_host, "idx_host or val_host is NULL");
    REQUIRE(k >= 1 && k <= s.n, "k must be in [1, %lld] (got %d)", (long long)s.n, (int)k);
    int32_t* idx = nullptr;
    double* val = nullptr;
    if ((rc = dmalloc(&idx, s.n * k)) || (rc = dmalloc(&val, s.n * k))) {
        (void)hipFree(idx);
        return rc;
    }
    const int grid = waves_grid(s.n);
    const double* S = s.S[s.cur];
    if (k <= 16)
        hipLaunchKernelGGL(topk_onepass_kernel<16>, dim3(grid), dim3(256), 0, p->stream, S, s.ld, s.n, k, exclude_diag,
                           idx, val);
    else if (k <= 32)
        hipLaunchKernelGGL(topk_onepass_kernel<32>, dim3(grid), dim3(256), 0, p->stream, S, s.ld, s.n, k, exclude_diag,
                           idx, val);
    else
        hipLaunchKernelGGL(topk_rounds_kernel, dim3(grid), dim3(256), 0, p->stream, S, s.ld, s.n, k, exclude_diag, idx,
                           val);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(idx_host, idx, size_t(s.n) * k * 4, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(val_host, val, size_t(s.n) * k * 8, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    (void)hipFree(idx);
    (void)hipFree(val);
    if (e != hipSuccess) {
        set_error("simrank_f64_plan_topk: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        return SIMRANK_F64_ERR_HIP;
    }
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_count_above(simrank_f64_plan* p, int32_t side, double t, int64_t* offsets_host) {
    int rc = side_ok(p, side);
    if (rc) return rc;
    REQUIRE(offsets_host, "offsets_host is NULL");
    REQUIRE(std::isfinite(t) && t > 0.0, "the threshold must be a finite number > 0 (got %g)", t);
    const Side& s = p->s[side];
    (void)hipFree(p->sel_off);
    p->sel_off = nullptr;
    p->sel_side = -1;
    int32_t* counts = nullptr;
    if ((rc = dmalloc(&counts, s.n))) return rc;
    hipLaunchKernelGGL(above_kernel<false>, dim3(waves_grid(s.n)), dim3(256), 0, p->stream, s.S[s.cur], s.ld, s.n, t,
                       counts, nullptr, 0, nullptr, nullptr);
    std::vector<int32_t> h((size_t)s.n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), counts, size_t(s.n) * 4, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    (void)hipFree(counts);
    if (e != hipSuccess) {
        set_error("simrank_f64_plan_count_above: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        return SIMRANK_F64_ERR_HIP;
    }
    offsets_host[0] = 0;
    for (int64_t r = 0; r < s.n; ++r) offsets_host[r + 1] = offsets_host[r] + h[(size_t)r];
    if ((rc = dmalloc(&p->sel_off, s.n + 1))) return rc;
    HIP_CHECK(hipMemcpyAsync(p->sel_off, offsets_host, size_t(s.n + 1) * 8, hipMemcpyHostToDevice, p->stream));
    HIP_CHECK(hipStreamSynchronize(p->stream));
    p->sel_side = side;
    p->sel_t = t;
    p->sel_n = offsets_host[s.n];
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_emit_above(simrank_f64_plan* p, int32_t side, double t, int64_t total, int32_t* ids_host,
                                double* vals_host) {
    int rc = side_ok(p, side);
    if (rc) return rc;
    REQUIRE(p->sel_side == side && p->sel_t == t && p->sel_off,
                "simrank_f64_plan_emit_above needs simrank_f64_plan_count_above of the same side and threshold first");
    REQUIRE(total == p->sel_n, "total %lld is not the count's %lld", (long long)total, (long long)p->sel_n);
    REQUIRE(total == 0 || (ids_host && vals_host), "ids_host or vals_host is NULL");
    if (total == 0) return SIMRANK_F64_OK;
    const Side& s = p->s[side];
    int32_t* ids = nullptr;
    double* vals = nullptr;
    if ((rc = dmalloc(&ids, total)) || (rc = dmalloc(&vals, total))) {
        (void)hipFree(ids);
        return rc;
    }
    hipLaunchKernelGGL(above_kernel<true>, dim3(waves_grid(s.n)), dim3(256), 0, p->stream, s.S[s.cur], s.ld, s.n, t,
                       nullptr, p->sel_off, total, ids, vals);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ids_host, ids, size_t(total) * 4, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(vals_host, vals, size_t(total) * 8, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    (void)hipFree(ids);
    (void)hipFree(vals);
    if (e != hipSuccess) {
        set_error("simrank_f64_plan_emit_above: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        return SIMRANK_F64_ERR_HIP;
    }
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_trim(simrank_f64_plan* p) {
    REQUIRE(p, "plan is NULL");
    (void)hipStreamSynchronize(p->stream);
    free_plan(p);
    p->released = true;
    return SIMRANK_F64_OK;
}

int simrank_f64_plan_get(const simrank_f64_plan* p, int32_t side, const char* key, int64_t* value) {
    REQUIRE(p && key && value, "plan, key or value is NULL");
    REQUIRE(side >= 0 && side < p->ns, "side %d out of range (the plan has %d)", (int)side, (int)p->ns);
    const Side& s = p->s[side];
    if (!std::strcmp(key, "iterate")) *value = p->released ? 0 : (int64_t)(uintptr_t)s.S[s.cur];
    else if (!std::strcmp(key, "iterate_ld")) *value = s.ld;
    else if (!std::strcmp(key, "iterate_rows")) *value = s.n;
    else REQUIRE(false, "unknown key '%s'", key);
    return SIMRANK_F64_OK;
}

}  // extern "C"
