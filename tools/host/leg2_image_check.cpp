// The padded id image of leg 2's short workgroups (api.hip build_short_image, common.h ShortImage), on the host alone
// under AddressSanitizer + UBSan (make -C simrank_amd/csrc leg2_image_check; the library's host logic compiled with
// -DSIMRANK_HOST_ONLY, as `make asan`).  For random row-pointer arrays — heavy-tailed, uniform, n < 64, all rows empty, a
// single tile, a heavy row that cuts its block — and both widths:
//   * the short groups are those of the rule, recomputed here from the tile list;
//   * every short tile is read back the way spmm.hip short_group3 reads it (tile record; per lane group the four
//     passes' scales, lengths, rows; per lane the ids of its slots) and gives: each row of the tile exactly once, in the
//     kernel's longest-first order (the order of its sort keys (length << 6 | row), descending), with its scale's bits and
//     its ids in CSR order, 0xFFFF in every slot past a row's end, zeros where a pass has no row;
//   * the records of every other tile are untouched (zeros, 0xFFFF).
// Exit code 0 = everything held.  No kernel is launched.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "common.h"

#define CHECK(c, ...)                                              \
    do {                                                           \
        if (!(c)) {                                                \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                          \
            fprintf(stderr, "\n");                                 \
            exit(1);                                               \
        }                                                          \
    } while (0)

struct Csr {
    int64_t n = 0;
    std::vector<int32_t> rowptr{0}, col;
    std::vector<float> scale;
};

static Csr from_lengths(std::mt19937& rng, const std::vector<int>& lengths) {
    Csr g;
    g.n = (int64_t)lengths.size();
    std::uniform_int_distribution<int32_t> any(0, (int32_t)std::max<int64_t>(1, g.n) - 1);
    for (int len : lengths) {
        for (int k = 0; k < len; ++k) g.col.push_back(any(rng));       // (the builder copies ids: they need not be distinct)
        std::sort(g.col.end() - len, g.col.end());
        g.rowptr.push_back((int32_t)g.col.size());
        g.scale.push_back(len ? 1.0f / float(len) : 0.f);
    }
    return g;
}

static int64_t g_short = 0, g_groups = 0;

static void check_graph(const Csr& g, const char* what) {
    const int64_t n = g.n, nnz = (int64_t)g.col.size();
    std::vector<int32_t> tile_row0, sym_map;
    const int64_t n_tiles = simrank::build_tiles(g.rowptr.data(), n, nnz, 2, tile_row0, sym_map, true);
    for (int width : {8, 16, 0, 12}) {
        simrank::ShortImage img;
        simrank::build_short_image(g.rowptr.data(), g.col.data(), g.scale.data(), n, tile_row0, n_tiles, width, img);
        // the rule
        const int64_t groups = (n_tiles + 3) / 4;
        std::vector<char> want((size_t)groups, 0);
        int64_t n_short = 0;
        if ((width == 8 || width == 16) && n >= 64)
            for (int64_t k = 0; k < groups; ++k) {
                bool ok = true;
                for (int64_t t = 4 * k; t < 4 * k + 4 && t < n_tiles; ++t) {
                    const int64_t lo = tile_row0[(size_t)t], hi = tile_row0[(size_t)t + 1];
                    if (lo % 32 != 0 || (hi != lo + 32 && hi != n)) ok = false;
                    for (int64_t a = lo; a < hi; ++a)
                        if (g.rowptr[(size_t)a + 1] - g.rowptr[(size_t)a] > width) ok = false;
                }
                want[(size_t)k] = ok;
                n_short += ok;
            }
        CHECK(img.groups == n_short, "%s, width %d: %d short groups, the rule says %lld", what, width, img.groups, (long long)n_short);
        if (n_short == 0) {
            CHECK(img.width == 0 && img.ids.empty() && img.meta.empty() && img.tiles.empty(), "%s, width %d: an image without short groups",
                  what, width);
            continue;
        }
        g_short += n_short;
        g_groups += groups;
        CHECK(img.width == width, "%s: width %d", what, img.width);
        const size_t tiles_pad = (size_t)groups * 4;
        const int nc = width / 8;
        CHECK(img.is_short.size() == (size_t)groups && img.tiles.size() == tiles_pad * 2 && img.meta.size() == tiles_pad * 64 &&
                  img.ids.size() == tiles_pad * 64 * (size_t)(width / 2),
              "%s, width %d: array sizes", what, width);
        for (size_t t = 0; t < tiles_pad; ++t) {
            const bool is_short = want[t / 4] && (int64_t)t < n_tiles;
            CHECK(!!img.is_short[t / 4] == !!want[t / 4], "%s, width %d: group %zu", what, width, t / 4);
            const uint16_t* ids = img.ids.data() + t * 64 * (size_t)(width / 2);
            const uint32_t* meta = img.meta.data() + t * 64;
            if (!is_short) {
                CHECK(img.tiles[2 * t] == 0 && img.tiles[2 * t + 1] == 0, "%s: tile %zu of no short group has a record", what, t);
                for (size_t i = 0; i < 64; ++i) CHECK(meta[i] == 0, "%s: tile %zu of no short group has lengths", what, t);
                for (size_t i = 0; i < 64 * (size_t)(width / 2); ++i) CHECK(ids[i] == 0xFFFF, "%s: tile %zu of no short group has ids", what, t);
                continue;
            }
            const int32_t row0 = img.tiles[2 * t], nrows = img.tiles[2 * t + 1];
            CHECK(row0 == tile_row0[t] && nrows == tile_row0[t + 1] - tile_row0[t] && nrows >= 1 && nrows <= 32 && row0 % 32 == 0,
                  "%s: tile %zu record (%d, %d)", what, t, row0, nrows);
            // the kernel's order: its sort keys, descending
            std::vector<int> keys;
            for (int r = 0; r < nrows; ++r) keys.push_back(((g.rowptr[(size_t)row0 + r + 1] - g.rowptr[(size_t)row0 + r]) << 6) | r);
            std::sort(keys.rbegin(), keys.rend());
            for (int s = 0; s < 32; ++s) {
                const int ps = s / 8, grp = s % 8;
                const uint32_t* m = meta + grp * 8;
                const int len = int((m[4] >> (8 * ps)) & 255u), row = int((m[5] >> (8 * ps)) & 255u);
                CHECK(m[6] == 0 && m[7] == 0, "%s: tile %zu spare words", what, t);
                if (s >= nrows) {
                    CHECK(len == 0 && row == 0 && m[ps] == 0, "%s: tile %zu pass %d group %d has no row but a record", what, t, ps, grp);
                } else {
                    CHECK(row == (keys[(size_t)s] & 63) && len == (keys[(size_t)s] >> 6), "%s: tile %zu sorted row %d is (%d, %d)", what, t,
                          s, row, len);
                    CHECK(std::memcmp(m + ps, g.scale.data() + row0 + row, 4) == 0, "%s: tile %zu row %d scale", what, t, row);
                }
                // as the kernel reads them: entry 8 c + q of the row from lane 8 grp + q, half-word ps * nc + c
                for (int j = 0; j < width; ++j) {
                    const int lane = 8 * grp + (j & 7), c = j >> 3;
                    const uint16_t id = ids[(size_t)lane * (size_t)(width / 2) + (size_t)(ps * nc + c)];
                    if (j < len)
                        CHECK(id == (uint16_t)g.col[(size_t)g.rowptr[(size_t)row0 + row] + (size_t)j], "%s: tile %zu row %d entry %d", what, t,
                              row, j);
                    else
                        CHECK(id == 0xFFFF, "%s: tile %zu sorted row %d slot %d is not padding", what, t, s, j);
                }
            }
        }
    }
}

int main() {
    std::mt19937 rng(20240611);
    std::uniform_real_distribution<double> u(0, 1);
    int graphs = 0;
    auto run = [&](const std::vector<int>& lengths, const char* what) {
        check_graph(from_lengths(rng, lengths), what);
        ++graphs;
    };
    for (int64_t n : {1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 500, 520, 1031, 2100}) {
        run(std::vector<int>((size_t)n, 0), "all rows empty");
        for (int rep = 0; rep < 6; ++rep) {
            std::vector<int> uni((size_t)n), heavy((size_t)n), edge((size_t)n);
            for (int64_t a = 0; a < n; ++a) {
                uni[(size_t)a] = (int)(u(rng) * 10);
                heavy[(size_t)a] = u(rng) < 0.1 ? 0 : (int)std::min<double>((double)std::min<int64_t>(n, 600), 2.0 / std::max(0.004, u(rng)));
                edge[(size_t)a] = (int)(std::vector<int>{0, 7, 8, 9, 15, 16, 17, 3})[(size_t)(u(rng) * 8) & 7];
            }
            run(uni, "uniform lengths 0..9");
            run(heavy, "heavy-tailed lengths");
            std::sort(heavy.begin(), heavy.end());
            run(heavy, "heavy-tailed lengths, ascending");
            // (runs of 128 equal lengths at the edges of both widths, then mixed)
            for (int64_t a = 0; a < n; ++a)
                if ((a / 128) % 2 == 0) edge[(size_t)a] = (int)(std::vector<int>{8, 9, 16, 17})[(size_t)(a / 256) & 3];
            run(edge, "lengths at the edges of both widths");
        }
    }
    printf("leg2_image_check: %d graphs, %lld short groups of %lld checked, all held\n", graphs, (long long)g_short, (long long)g_groups);
    CHECK(g_short > 0, "no short group was ever built");
    return 0;
}
