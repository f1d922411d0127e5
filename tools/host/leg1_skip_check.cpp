// The one-matrix plan's node order and its table of leg-1 units that a triangle-form leg 2 never reads (planprep.hip:
// refine_by_first_reference, first_block_table), on the host alone under AddressSanitizer + UBSan
// (make -C simrank_amd/csrc leg1_skip_check; the library's host logic compiled with -DSIMRANK_HOST_ONLY, as `make asan`).
// For random and degenerate graphs:
//   * the order is a permutation, ascending in row length, and (reorder) ties are in the order of first(i) under the order
//     of the pass before — checked as: a second, independent run gives the same order (plan_prepare is deterministic, also
//     where `renamed` takes its threads: the large graph below), and reorder = 0 keeps the caller's order;
//   * first_block equals a brute-force recomputation from the renamed pattern;
//   * for every unit (128-row block b, panel P) with b < first_block[P], no (row a, panel q) pair that leg 2 computes reads
//     one of its elements Tt[i, 128 b ..], i in panel P.  Leg 2's pairs are enumerated as its launches do:
//       - gather3_kernel<kSym> with the balanced tile list: workgroup (panel, rt) of sym_map, wave w -> tile 4 rt + w =
//         rows [tile_row0[t], tile_row0[t + 1]), computed iff (row0 & ~31) <= 32 panel;
//       - the same kernel without a list: 32-row tiles t, panels with 32 t <= 32 panel;
//       - fused_trans_kernel<., SYM>: 128-row block B computes panel q iff B <= (32 q + 31) >> 7.
// Exit code 0 = everything held.  No kernel is launched.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
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
    int64_t n;
    std::vector<int32_t> rowptr, col;
    std::vector<float> scale;
};

static Csr from_rows(const std::vector<std::set<int32_t>>& rows) {
    Csr g{(int64_t)rows.size(), {0}, {}, {}};
    for (const auto& r : rows) {
        for (int32_t c : r) g.col.push_back(c);
        g.rowptr.push_back((int32_t)g.col.size());
        g.scale.push_back(r.empty() ? 0.f : 1.0f / float(r.size()));
    }
    return g;
}

// heavy-tailed row lengths, columns drawn towards a few hubs; empty rows and unreferenced nodes occur
static Csr powerlaw(std::mt19937& rng, int64_t n, double avg) {
    std::vector<std::set<int32_t>> rows((size_t)n);
    std::uniform_real_distribution<double> u(0, 1);
    for (int64_t a = 0; a < n; ++a) {
        if (u(rng) < 0.1) continue;
        const int d = (int)std::min<double>((double)n, avg * 0.5 / std::max(0.02, u(rng)));
        for (int k = 0; k < d; ++k) {
            const double x = u(rng);
            rows[(size_t)a].insert((int32_t)std::min<double>((double)n - 1, x * x * x * (double)n));
        }
    }
    return from_rows(rows);
}

static Csr uniform(std::mt19937& rng, int64_t n, int deg) {
    std::vector<std::set<int32_t>> rows((size_t)n);
    std::uniform_int_distribution<int32_t> any(0, (int32_t)n - 1);
    for (int64_t a = 0; a < n; ++a)
        for (int k = 0; k < deg; ++k) rows[(size_t)a].insert(any(rng));
    return from_rows(rows);
}

static int64_t g_units_dead = 0, g_units = 0;

static void check_graph(const Csr& g, const char* what, bool reorder) {
    const int64_t n = g.n, nnz = (int64_t)g.col.size();
    simrank_plan_options opt{};
    opt.coef = 0.8f;
    opt.reorder = reorder ? 1 : 0;
    opt.dense_terms = 3;
    simrank::PlanPrep pp, again;
    CHECK(simrank::plan_prepare(n, nnz, g.rowptr.data(), g.col.data(), g.scale.data(), &opt, &pp) == SIMRANK_OK,
          "%s: plan_prepare: %s", what, simrank_last_error());
    CHECK(simrank::plan_prepare(n, nnz, g.rowptr.data(), g.col.data(), g.scale.data(), &opt, &again) == SIMRANK_OK,
          "%s: plan_prepare (again)", what);
    CHECK(pp.ord == again.ord && pp.inv == again.inv && pp.first_block == again.first_block && pp.rp == again.rp &&
              pp.cl == again.cl,
          "%s: two runs differ", what);
    // a permutation, ascending in length
    std::vector<int> seen((size_t)n, 0);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t a = pp.ord[(size_t)r];
        CHECK(a >= 0 && a < n && !seen[(size_t)a]++, "%s: order is not a permutation at %lld", what, (long long)r);
        CHECK(pp.inv[(size_t)a] == r, "%s: inv is not the inverse at %lld", what, (long long)r);
        if (!reorder) CHECK(a == r, "%s: reorder = 0 moved node %d", what, a);
        const int32_t len = g.rowptr[a + 1] - g.rowptr[a];
        CHECK(pp.rp[(size_t)r + 1] - pp.rp[(size_t)r] == len, "%s: renamed row %lld has another length", what, (long long)r);
        if (reorder && r > 0) {
            const int32_t b = pp.ord[(size_t)r - 1];
            CHECK(g.rowptr[b + 1] - g.rowptr[b] <= len, "%s: lengths not ascending at %lld", what, (long long)r);
        }
    }
    // the table against brute force: for every node, scan the rows in order
    const int64_t npan = (n + 31) / 32, nblk = (n + 127) / 128;
    CHECK((int64_t)pp.first_block.size() == npan, "%s: table of %zu panels", what, pp.first_block.size());
    std::vector<int32_t> brute((size_t)npan, simrank::kLeg1Never);
    for (int64_t i = 0; i < n; ++i) {
        int64_t first = -1;
        for (int64_t a = 0; a < n && first < 0; ++a)
            if (std::binary_search(pp.cl.begin() + pp.rp[(size_t)a], pp.cl.begin() + pp.rp[(size_t)a + 1], (int32_t)i)) first = a;
        if (first >= 0) brute[(size_t)(i >> 5)] = std::min<int32_t>(brute[(size_t)(i >> 5)], (int32_t)(first / 128));
    }
    CHECK(brute == pp.first_block, "%s: first_block differs from brute force", what);
    for (int64_t P = 0; P < npan; ++P) {
        g_units += nblk;
        g_units_dead += std::min<int64_t>(nblk, pp.first_block[(size_t)P]);
    }
    // what leg 2 reads: row a computing panel q reads Tt[i, panel q] for i in N(a) = an element of leg 1's unit
    // (block q / 4, panel i / 32)
    auto reads = [&](int64_t a, int64_t q, const char* form) {
        for (int32_t j = pp.rp[(size_t)a]; j < pp.rp[(size_t)a + 1]; ++j) {
            const int32_t i = pp.cl[(size_t)j];
            CHECK(q / 4 >= pp.first_block[(size_t)(i >> 5)], "%s: %s row %lld, panel %lld reads Tt[%d, .] of skipped unit (%lld, %d)", what,
                  form, (long long)a, (long long)q, i, (long long)(q / 4), i >> 5);
        }
    };
    for (int64_t balance : {int64_t(2), int64_t(0)}) {
        std::vector<int32_t> tile_row0, sym_map;
        const int64_t n_tiles = simrank::build_tiles(pp.rp.data(), n, nnz, balance, tile_row0, sym_map, true);
        if (n_tiles && !sym_map.empty()) {
            std::vector<std::vector<char>> done((size_t)n_tiles, std::vector<char>((size_t)npan, 0));
            for (size_t w = 0; w < sym_map.size() / 2; ++w) {
                const int64_t panel = sym_map[2 * w], rt = sym_map[2 * w + 1];
                if (panel < 0) continue;
                CHECK(panel < npan, "%s: launch list names panel %lld", what, (long long)panel);
                for (int wave = 0; wave < 4; ++wave) {
                    const int64_t t = rt * 4 + wave;
                    if (t >= n_tiles) continue;
                    const int64_t row0 = tile_row0[(size_t)t], row1 = tile_row0[(size_t)t + 1];
                    if ((row0 & ~int64_t(31)) > 32 * panel) continue;          // (rb > c0: nothing computed)
                    done[(size_t)t][(size_t)panel] = 1;
                    for (int64_t a = row0; a < row1; ++a) reads(a, panel, "gather (tile list)");
                }
            }
            // ... and the list leaves out no tile on or above the diagonal (or the enumeration above proves nothing)
            for (int64_t t = 0; t < n_tiles; ++t)
                for (int64_t q = tile_row0[(size_t)t] / 32; q < npan; ++q)
                    CHECK(done[(size_t)t][(size_t)q], "%s: tile %lld, panel %lld is in no workgroup", what, (long long)t, (long long)q);
        } else {
            for (int64_t t = 0; t < npan; ++t)
                for (int64_t q = t; q < npan; ++q)
                    for (int64_t a = 32 * t; a < std::min(n, 32 * t + 32); ++a) reads(a, q, "gather (uniform tiles)");
        }
    }
    for (int64_t B = 0; B < nblk; ++B)
        for (int64_t q = 0; q < npan; ++q) {
            if (B > ((32 * q + 31) >> 7)) continue;                            // (n_sub_sym <= 0)
            for (int64_t a = 128 * B; a < std::min(n, 128 * B + 128); ++a) reads(a, q, "one-launch leg 2");
        }
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 40;
    std::mt19937 rng(20240607);
    // (the refined order at every size: by default plan_prepare keeps the stable length order below 16384 nodes)
    CHECK(simrank_set_tuning("leg1_order", 1) == SIMRANK_OK, "leg1_order: %s", simrank_last_error());
    // degenerate graphs
    for (int64_t n : {int64_t(1), int64_t(31), int64_t(64), int64_t(128), int64_t(129), int64_t(300)}) {
        std::vector<std::set<int32_t>> rows((size_t)n);
        for (bool reorder : {true, false}) check_graph(from_rows(rows), "no entries", reorder);
        for (int64_t c = 0; c < n; ++c) rows[0].insert((int32_t)c);
        for (bool reorder : {true, false}) check_graph(from_rows(rows), "row 0 references everything", reorder);
        rows[0].clear();
        for (int64_t a = std::max<int64_t>(0, n - 20); a < n; ++a)
            for (int64_t c = 0; c < n; c += 1 + a % 3) rows[(size_t)a].insert((int32_t)c);
        for (bool reorder : {true, false}) check_graph(from_rows(rows), "only the last rows reference anything", reorder);
        for (int64_t a = 0; a < n; ++a) rows[(size_t)a] = {(int32_t)a};
        for (bool reorder : {true, false}) check_graph(from_rows(rows), "self loops only", reorder);
    }
    for (int it = 0; it < rounds; ++it) {
        const int64_t n = 40 + int64_t(rng() % 1400);
        char what[64];
        snprintf(what, sizeof what, "power law %d (n = %lld)", it, (long long)n);
        const Csr g = powerlaw(rng, n, 2.0 + double(rng() % 6));
        check_graph(g, what, true);
        if (it % 4 == 0) check_graph(g, what, false);
        snprintf(what, sizeof what, "uniform %d (n = %lld)", it, (long long)n);
        check_graph(uniform(rng, n, 1 + int(rng() % 8)), what, true);
    }
    // large enough for the threads of `renamed` (100 000 entries): the same order from every run
    check_graph(uniform(rng, 2600, 48), "uniform, 2600 x 48", true);
    CHECK(g_units_dead > 0, "no graph had a dead unit: the checks above proved nothing");
    printf("leg1_skip_check: ok, %lld of %lld units dead over all graphs\n", (long long)g_units_dead, (long long)g_units);
    return 0;
}
