// Stand-alone check of csrc/affine_plan.hpp (tests/test_affine_plan.py builds it with the address and undefined-behaviour sanitizers and
// runs it): seeded random batches against the properties the kernels and the host drivers of both gap-affine batches rely on, for the
// two-layer layout and the four-layer layout at 16 rows per lane; for 8 rows per lane only the sizes, against the formulas.  The formulas
// the header is compared with are written out here, not taken from it.  Exit status 0 and "ok <batches> <chunks> <states>" when every
// property held, else the first violation on stderr and status 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "affine_plan.hpp"

using namespace pa::affine_plan;

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            std::fprintf(stderr, "%s, batch %d: ", lname, batch);   \
            std::fprintf(stderr, __VA_ARGS__);                      \
            std::fprintf(stderr, " (%s)\n", #cond);                 \
            return false;                                           \
        }                                                           \
    } while (0)

namespace {

typedef std::pair<size_t, size_t> Range;  // [begin, end)

// The formulas, written out: R rows per lane, S = 64 R rows per strip.
size_t ref_lg(const Layout& L, size_t m) {
    size_t lg = 0;
    while (L.rows * (size_t(1) << lg) < m) ++lg;
    return lg;
}
size_t ref_strips(const Layout& L, size_t m) { return m <= 64 * L.rows ? 1 : (m + 64 * L.rows - 1) / (64 * L.rows); }
size_t ref_H(const Layout& L, size_t m) { return m <= 64 * L.rows ? L.rows * (size_t(1) << ref_lg(L, m)) : ref_strips(L, m) * 64 * L.rows; }
size_t ref_K(size_t n, size_t C) { return n ? (n - 1) / C : 0; }
size_t ref_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
size_t ref_code_bytes(const Layout& L, size_t n, size_t m) { return ref_up((n + 1) * (ref_H(L, m) + 1), 16); }
size_t ref_ckpt_bytes(const Layout& L, size_t n, size_t m, size_t C) { return ref_up(ref_K(n, C) * (ref_H(L, m) + 1) * L.ck_row_bytes, L.ck_align); }
size_t ref_rowck_bytes(const Layout& L, size_t n, size_t m) { return (ref_strips(L, m) - 1) * (n + 1) * L.bnd_bytes; }
size_t ref_Ht(const Layout& L, size_t m) { return std::min<size_t>(ref_H(L, m), 64 * L.rows); }
size_t ref_tile_bytes(const Layout& L, size_t n, size_t m, size_t C) { return ref_up((std::min(n, C) + 1) * (ref_Ht(L, m) + 1), 16); }
size_t ref_tiled_bytes(const Layout& L, size_t n, size_t m, size_t C) {
    return ref_rowck_bytes(L, n, m) + ref_ckpt_bytes(L, n, m, C) + ref_tile_bytes(L, n, m, C) + n + m;
}
size_t ref_visits(const Layout& L, size_t n, size_t m, size_t C) { return (n + C - 1) / C + (std::max<size_t>(m, 1) + 64 * L.rows - 1) / (64 * L.rows); }

bool disjoint_inside(std::vector<Range> r, size_t size) {
    std::sort(r.begin(), r.end());
    for (size_t x = 0; x < r.size(); ++x)
        if (r[x].first > r[x].second || r[x].second > size || (x && r[x - 1].second > r[x].first)) return false;
    return true;
}

// A length in 0 .. 5000: uniform, or an edge of a packed width, of the strip height or of a tile width (+-1), or 0 or 1.
uint32_t random_len(std::mt19937_64& rng, const Layout& L) {
    switch (rng() % 4) {
        case 0: {
            const uint32_t k = (uint32_t)(rng() % 10);  // rows 2^k, k <= 6; then 2, 3 and 4 strips
            const uint32_t edge = k <= 6 ? L.rows << k : (k - 5) * 64 * L.rows;
            return std::min<uint32_t>(5000, edge - 1 + (uint32_t)(rng() % 3));
        }
        case 1: return (uint32_t)(rng() % 3) == 0 ? (uint32_t)(rng() % 2) : (uint32_t)(rng() % 201);
        default: return (uint32_t)(rng() % 5001);
    }
}

struct Totals {
    long long chunks = 0, states = 0;
};

// The sizes against the formulas; all that is checked for 8 rows per lane.
bool check_sizes(const char* lname, int batch, const Layout& L, uint32_t n, uint32_t m, uint32_t C) {
    CHECK((size_t)seg_lg(L, m) == ref_lg(L, m) || m > 64 * L.rows, "seg_lg(%u)", m);
    CHECK(strips_of(L, m) == ref_strips(L, m), "strips_of(%u) = %zu", m, strips_of(L, m));
    CHECK(rows_of(L, m) == ref_H(L, m), "rows_of(%u) = %zu", m, rows_of(L, m));
    CHECK(rows_of(L, m) >= m && rows_of(L, m) % L.rows == 0, "rows_of(%u) = %zu", m, rows_of(L, m));
    CHECK(code_bytes_of(L, n, m) == ref_code_bytes(L, n, m), "code_bytes_of(%u, %u)", n, m);
    CHECK(ckpt_cols_of(n, C) == ref_K(n, C), "ckpt_cols_of(%u, %u)", n, C);
    CHECK(ckpt_bytes_of(L, n, m, C) == ref_ckpt_bytes(L, n, m, C), "ckpt_bytes_of(%u, %u, %u)", n, m, C);
    CHECK(tile_rows_of(L, m) == ref_Ht(L, m), "tile_rows_of(%u)", m);
    CHECK(tile_bytes_of(L, n, m, C) == ref_tile_bytes(L, n, m, C), "tile_bytes_of(%u, %u, %u)", n, m, C);
    CHECK(tiled_bytes_of(L, n, m, C) == ref_tiled_bytes(L, n, m, C), "tiled_bytes_of(%u, %u, %u) = %zu", n, m, C, tiled_bytes_of(L, n, m, C));
    CHECK(tile_visits_max(L, n, m, C) == ref_visits(L, n, m, C), "tile_visits_max(%u, %u, %u)", n, m, C);
    return true;
}

// One state of a walk: the tile job's reads stay inside the pair's checkpoints, its tile inside the tile buffer.
bool check_state(const char* lname, int batch, const Layout& L, uint32_t n, uint32_t m, uint32_t C, uint32_t i, uint32_t j) {
    const size_t S = 64 * L.rows, H = ref_H(L, m), K = ref_K(n, C), Ht = ref_Ht(L, m);
    const TileGeom G = tile_geom(L, n, m, C, i, j);
    const uint32_t cs = G.c0 ? G.c0 + 1 : 0;
    CHECK(G.ct == (i ? (i - 1) / C : 0) && G.rt == (j ? (j - 1) / S : 0) && G.c0 == G.ct * C, "tile (%u, %u) of state (%u, %u)", G.ct, G.rt, i, j);
    CHECK(cs <= G.c1 && G.c1 == i, "columns %u .. %u of state (%u, %u)", cs, G.c1, i, j);
    CHECK(G.cols == G.c1 - cs + 1 && G.steps == G.cols + G.rlast, "cols %u, steps %u", G.cols, G.steps);
    CHECK(G.rlast < 64, "rlast %u of state (%u, %u)", G.rlast, i, j);
    CHECK(G.Ht == Ht && G.rt * S + Ht <= H, "Ht %u of %zu rows", G.Ht, H);
    if (j) CHECK(j > G.rt * S && j <= G.rt * S + Ht && (j - 1 - G.rt * S) / L.rows == G.rlast, "row %u in row tile %u, lane %u", j, G.rt, G.rlast);
    // the tile buffer: cols columns of Ht rows, then row 0 of every column
    CHECK(G.cols <= std::min<size_t>(n, C) + 1, "%u columns in a tile of C = %u", G.cols, C);
    CHECK((size_t)G.cols * Ht <= G.row0 && (size_t)G.row0 + G.cols <= ref_tile_bytes(L, n, m, C), "tile of %u x %zu, row 0 at %u of %zu bytes", G.cols, Ht,
          G.row0, ref_tile_bytes(L, n, m, C));
    if (G.ct) {  // the strip's rows of the checkpoint at c0, and its row 0 (behind the K H rows)
        CHECK(G.ct <= K, "column tile %u of %zu checkpoints", G.ct, K);
        CHECK(G.left_off % L.ck_row_bytes == 0 && G.left_off + Ht * L.ck_row_bytes <= K * H * L.ck_row_bytes, "left at %zu", G.left_off);
        CHECK(G.left_off == ((size_t)(G.ct - 1) * H + G.rt * S) * L.ck_row_bytes, "left at %zu", G.left_off);
        CHECK(G.left0_off == (K * H + G.ct - 1) * L.ck_row_bytes && G.left0_off + L.ck_row_bytes <= ref_ckpt_bytes(L, n, m, C), "left0 at %zu", G.left0_off);
    }
    if (G.rt) CHECK(G.above_off == (size_t)(G.rt - 1) * (n + 1) * L.bnd_bytes && G.above_off + (size_t)(n + 1) * L.bnd_bytes <= ref_rowck_bytes(L, n, m),
                    "above at %zu of %zu", G.above_off, ref_rowck_bytes(L, n, m));
    CHECK(G.packed == (m <= S) && G.lg == (G.packed ? ref_lg(L, m) : 6), "lg %u", G.lg);
    CHECK(G.refill_cells == (double)G.cols * L.rows * (G.rlast + 1), "refill_cells");
    return true;
}

// The plan of one chunk (or of the whole batch: Keep::kNone).
bool check_plan(const char* lname, int batch, const Layout& L, const std::vector<uint32_t>& n, const std::vector<uint32_t>& m,
                const std::vector<uint32_t>& ids, Keep keep, uint32_t C) {
    const Waves P = plan_waves(L, n, m, ids, keep, C);
    CHECK(P.pairs.size() == ids.size(), "%zu slots for %zu pairs", P.pairs.size(), ids.size());
    for (size_t k = 0; k < ids.size(); ++k) CHECK(P.pairs[k].id == ids[k], "slot %zu holds pair %u", k, P.pairs[k].id);
    // the waves tile the slots; one width per wave, at most 64 / g pairs, a multi-strip wave exactly one
    std::vector<WaveSlot> by_first = P.waves;
    std::sort(by_first.begin(), by_first.end(), [](const WaveSlot& x, const WaveSlot& y) { return x.first < y.first; });
    size_t next = 0, packed = 0;
    std::vector<Range> bnd;
    for (const WaveSlot& W : by_first) {
        CHECK(W.first == next && W.np >= 1 && W.np <= (64u >> W.lg), "wave at %u with %u pairs of width 2^%u", W.first, W.np, W.lg);
        uint32_t nmax = 0;
        for (uint32_t k = W.first; k < W.first + W.np; ++k) {
            const uint32_t p = P.pairs[k].id;
            CHECK((m[p] <= 64 * L.rows ? ref_lg(L, m[p]) : 6) == W.lg && ref_strips(L, m[p]) == W.strips, "pair %u (|b| = %u) in a wave of lg %u, %u strips", p,
                  m[p], W.lg, W.strips);
            CHECK(P.pairs[k].H == ref_H(L, m[p]) && P.pairs[k].lg == W.lg, "pair %u: H %u, lg %u", p, P.pairs[k].H, P.pairs[k].lg);
            nmax = std::max(nmax, n[p]);
            packed += m[p] <= 64 * L.rows;
        }
        CHECK(W.nmax == nmax, "nmax %u, expected %u", W.nmax, nmax);
        CHECK((W.strips > 1) == (W.bnd_off != SIZE_MAX), "a wave of %u strips has boundary rows or a one-strip wave has them", W.strips);
        if (W.strips > 1) {
            // a multi-strip wave holds one pair, so its rows sized by nmax (the plan) are its rows sized by n (tiled_bytes_of, the budget)
            CHECK(W.np == 1 && W.nmax == n[P.pairs[W.first].id], "a multi-strip wave of %u pairs", W.np);
            const size_t rows = keep == Keep::kCkpt ? W.strips - 1 : 1, bytes = rows * ((size_t)W.nmax + 1) * L.bnd_bytes;
            if (keep == Keep::kCkpt) CHECK(bytes == ref_rowck_bytes(L, n[P.pairs[W.first].id], m[P.pairs[W.first].id]), "row checkpoints of %zu bytes", bytes);
            CHECK(W.bnd_off % L.bnd_bytes == 0, "boundary rows at %zu", W.bnd_off);
            bnd.push_back(Range(W.bnd_off, W.bnd_off + bytes));
        }
        next += W.np;
    }
    CHECK(next == ids.size() && packed == P.packed && ids.size() - packed == P.strip, "waves cover %zu of %zu slots", next, ids.size());
    CHECK(disjoint_inside(bnd, P.bnd_vals * L.bnd_bytes), "boundary rows overlap or leave their %zu bytes", P.bnd_vals * L.bnd_bytes);
    for (size_t w = 1; w < P.waves.size(); ++w) {
        const WaveSlot &x = P.waves[w - 1], &y = P.waves[w];
        CHECK((uint64_t)x.strips * (x.nmax + (1u << x.lg)) >= (uint64_t)y.strips * (y.nmax + (1u << y.lg)), "wave %zu costs more than the wave before it", w);
    }
    // codes or column checkpoints, tiles and ops: disjoint, inside their allocations, aligned
    std::vector<Range> data, tiles, ops;
    size_t sum_tiled = 0;
    for (const PairSlot& q : P.pairs) {
        const uint32_t p = q.id;
        const size_t bytes = keep == Keep::kCodes ? ref_code_bytes(L, n[p], m[p]) : keep == Keep::kCkpt ? ref_ckpt_bytes(L, n[p], m[p], C) : 0;
        CHECK(q.data_off % (keep == Keep::kCkpt ? L.ck_align : 16) == 0, "pair %u: codes or checkpoints at %zu", p, q.data_off);
        data.push_back(Range(q.data_off, q.data_off + bytes));
        if (keep != Keep::kNone) ops.push_back(Range(q.ops_off, q.ops_off + n[p] + m[p]));
        if (keep == Keep::kCkpt) {
            CHECK(q.tile_off % 16 == 0, "pair %u: tile at %zu", p, q.tile_off);
            tiles.push_back(Range(q.tile_off, q.tile_off + ref_tile_bytes(L, n[p], m[p], C)));
            sum_tiled += ref_tiled_bytes(L, n[p], m[p], C);
        }
    }
    CHECK(disjoint_inside(data, P.data_bytes), "codes or checkpoints overlap or leave their %zu bytes", P.data_bytes);
    CHECK(disjoint_inside(ops, P.ops_bytes), "ops overlap or leave their %zu bytes", P.ops_bytes);
    CHECK(disjoint_inside(tiles, P.tile_bytes), "tiles overlap or leave their %zu bytes", P.tile_bytes);
    if (keep == Keep::kCkpt)
        CHECK(P.data_bytes + P.bnd_vals * L.bnd_bytes + P.tile_bytes + P.ops_bytes <= sum_tiled, "the chunk occupies more than the %zu bytes it was charged",
              sum_tiled);
    return true;
}

bool check_layout(const char* lname, const Layout& L, bool sizes_only, int batches, uint64_t seed, Totals& T) {
    std::mt19937_64 rng(seed);
    const uint32_t tile_cols[3] = {64, 256, 1024};
    for (int batch = 0; batch < batches; ++batch) {
        const size_t np = 1 + rng() % 24;
        const uint32_t C = tile_cols[batch % 3];
        std::vector<uint32_t> n(np), m(np);
        for (size_t p = 0; p < np; ++p) {
            n[p] = rng() % 6 == 0 ? std::min<uint32_t>(5000, (uint32_t)(1 + rng() % 3) * C - 1 + (uint32_t)(rng() % 3)) : random_len(rng, L);
            m[p] = random_len(rng, L);
            if (!check_sizes(lname, batch, L, n[p], m[p], C)) return false;
        }
        if (sizes_only) continue;
        // the planner's order: packed pairs by (width, |a|), then strip pairs by |a|; a permutation, ties in the order given
        const std::vector<uint32_t> order = planner_order(L, n, m);
        std::vector<uint32_t> seen = order;
        std::sort(seen.begin(), seen.end());
        for (size_t p = 0; p < np; ++p) CHECK(seen.size() == np && seen[p] == p, "the order is no permutation");
        for (size_t k = 1; k < np; ++k) {
            const uint32_t x = order[k - 1], y = order[k];
            const size_t gx = m[x] <= 64 * L.rows ? ref_lg(L, m[x]) : 7, gy = m[y] <= 64 * L.rows ? ref_lg(L, m[y]) : 7;
            CHECK(gx < gy || (gx == gy && (n[x] < n[y] || (n[x] == n[y] && x < y))), "pairs %u and %u out of order", x, y);
        }
        if (!check_plan(lname, batch, L, n, m, order, Keep::kNone, 0)) return false;
        // the chunks of align() (by codes) and of align_tiled() (by checkpoints, tile and ops), from one chunk down to the largest pair alone
        for (int tiled = 0; tiled < 2; ++tiled) {
            auto size_of = [&](uint32_t p) { return tiled ? ref_tiled_bytes(L, n[p], m[p], C) : ref_code_bytes(L, n[p], m[p]); };
            size_t total = 0, biggest = 0;
            for (uint32_t p = 0; p < np; ++p) total += size_of(p), biggest = std::max(biggest, size_of(p));
            const size_t budget = batch % 4 == 0 ? total : batch % 4 == 1 ? biggest : std::max(biggest, total / (2 + rng() % 6));
            size_t nchunks = 0;
            for (size_t c0 = 0, bytes; c0 < np;) {
                const std::vector<uint32_t> ids = next_chunk(order, c0, budget, size_of, &bytes);
                CHECK(!ids.empty() && c0 + ids.size() <= np, "a chunk of %zu pairs at %zu", ids.size(), c0);
                size_t sum = 0;
                for (size_t k = 0; k < ids.size(); ++k) {
                    CHECK(ids[k] == order[c0 + k], "chunk at %zu: pair %u", c0, ids[k]);
                    sum += size_of(ids[k]);
                }
                CHECK(sum == bytes && bytes <= budget, "a chunk of %zu bytes (sum %zu) at a budget of %zu", bytes, sum, budget);  // (every pair fits)
                if (c0 + ids.size() < np) CHECK(bytes + size_of(order[c0 + ids.size()]) > budget, "the chunk at %zu stops early", c0);
                if (!check_plan(lname, batch, L, n, m, ids, tiled ? Keep::kCkpt : Keep::kCodes, tiled ? C : 0)) return false;
                c0 += ids.size();
                ++nchunks;
            }
            if (batch % 4 == 0) CHECK(nchunks == 1, "%zu chunks at a budget of the total", nchunks);
            T.chunks += (long long)nchunks;
        }
        for (size_t p = 0; p < np; ++p) {
            // every state but (0, 0); of a pair beyond 200 x 200 the borders of its tiles and a random sample
            if (n[p] <= 200 && m[p] <= 200) {
                for (uint32_t i = 0; i <= n[p]; ++i)
                    for (uint32_t j = i ? 0 : 1; j <= m[p]; ++j, ++T.states)
                        if (!check_state(lname, batch, L, n[p], m[p], C, i, j)) return false;
            } else {
                for (int k = 0; k < 400; ++k, ++T.states) {
                    uint32_t i = (uint32_t)(rng() % ((uint64_t)n[p] + 1)), j = (uint32_t)(rng() % ((uint64_t)m[p] + 1));
                    if (k % 4 == 1) i = std::min<uint32_t>(n[p], (i / C) * C + (uint32_t)(rng() % 2));           // a tile's last column, the next one's first
                    if (k % 4 == 2) j = std::min<uint32_t>(m[p], (j / (64 * L.rows)) * 64 * L.rows + (uint32_t)(rng() % 2));  // the same for rows
                    if (k % 4 == 3) i = n[p], j = m[p] - std::min<uint32_t>(m[p], k / 4);
                    if (i == 0 && j == 0) j = m[p] ? 1 : 0, i = m[p] ? 0 : std::min<uint32_t>(n[p], 1);
                    if (i == 0 && j == 0) continue;  // (the empty pair has no state to walk)
                    if (!check_state(lname, batch, L, n[p], m[p], C, i, j)) return false;
                }
            }
            // the staircase from (n, m): every move leaves the tile, by its first column and by its first row in turn
            uint32_t i = n[p], j = m[p], visits = 0;
            for (bool left = true; i || j; left = !left) {
                ++visits;
                CHECK(visits <= tile_visits_max(L, n[p], m[p], C), "the staircase of (%u, %u) visits more than %u tiles", n[p], m[p],
                      tile_visits_max(L, n[p], m[p], C));
                const TileGeom G = tile_geom(L, n[p], m[p], C, i, j);
                if ((left && i) || !j) i = G.c0;
                else j = G.rt * 64 * L.rows;
            }
        }
    }
    return true;
}

}  // namespace

int main() {
    const Layout two{16, 8, 8, 8}, four{16, 16, 12, 16}, four8{8, 16, 12, 16};
    const int batches = 300;
    Totals T;
    if (!check_layout("two-layer", two, false, batches, 20240611, T) || !check_layout("four-layer", four, false, batches, 20240612, T) ||
        !check_layout("four-layer, 8 rows", four8, true, batches, 20240613, T))
        return 1;
    // two values of the formulas as they stood before this header existed
    if (tiled_bytes_of(two, 3000, 3000, 256) != 587880 || tiled_bytes_of(four, 3000, 3000, 256) != 771120) {
        std::fprintf(stderr, "tiled_bytes_of(3000, 3000, 256) = %zu, %zu\n", tiled_bytes_of(two, 3000, 3000, 256), tiled_bytes_of(four, 3000, 3000, 256));
        return 1;
    }
    std::printf("ok %d %lld %lld\n", 3 * batches, T.chunks, T.states);
    return 0;
}
