// affine_plan.hpp -- the host-side plan and tile geometry of both gap-affine batches (two layers: affine_unit.hip; four layers:
// affine4_unit.hip, affine4_tiled_unit.hip).  Plain C++, no HIP, no device pointers: offsets and counts only, which affine_host.hpp turns
// into the kernels' records.  tests/test_affine_plan.py compiles it on its own.
//
// A batch type describes itself by a Layout.  A lane owns `rows` rows of b, a wavefront 64 lanes: pairs with |b| <= 64 rows are packed,
// 64 / g of one segment width g = 2^lg per wavefront, H = g rows rows each; longer ones are cut into strips of 64 rows rows, a wavefront
// per pair, H = strips 64 rows.  The tiled traceback ("Tiled traceback") keeps, per pair, the boundary row of every
// strip but the last (row checkpoints) and every C-th column (column checkpoints), and re-fills one tile of codes at a time.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pa {
namespace affine_plan {

struct Layout {
    uint32_t rows;          // rows of b per lane
    uint32_t bnd_bytes;     // one value of a boundary row
    uint32_t ck_row_bytes;  // one row of a column checkpoint
    uint32_t ck_align;      // a pair's column checkpoints are rounded up to this many bytes
};

// Column tiles of 1024 columns are as wide as the row tiles (a strip of 64 x 16 rows) are high: the row and the column checkpoints then
// cost the same |a| |b| / 128 bytes each, a tile of codes is 1 MiB, and a path near the diagonal crosses about as many column edges as
// row edges.
constexpr uint32_t kTileColsDefault = 1024, kTileColsMin = 64, kTileColsMax = 1u << 20;

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline size_t strip_rows(const Layout& L) { return size_t(64) * L.rows; }  // rows of one strip
inline bool packed(const Layout& L, uint32_t m) { return m <= strip_rows(L); }
inline int seg_lg(const Layout& L, size_t m) {  // log2 of the segment width: smallest g = 2^lg with g rows >= m
    int lg = 0;
    while ((size_t(L.rows) << lg) < m) ++lg;
    return lg;
}
inline size_t strips_of(const Layout& L, uint32_t m) { return packed(L, m) ? 1 : (m + strip_rows(L) - 1) / strip_rows(L); }
inline size_t rows_of(const Layout& L, uint32_t m) { return packed(L, m) ? size_t(L.rows) << seg_lg(L, m) : strips_of(L, m) * strip_rows(L); }  // H

// A pair's sizes, each by H = rows_of(m) for a caller that has it (a wave's pairs share one H) and by m.
inline size_t code_bytes_h(uint32_t n, size_t H) { return round_up(((size_t)n + 1) * (H + 1), 16); }
inline size_t code_bytes_of(const Layout& L, uint32_t n, uint32_t m) { return code_bytes_h(n, rows_of(L, m)); }
inline size_t ckpt_cols_of(uint32_t n, uint32_t C) { return n ? (n - 1) / C : 0; }  // checkpointed columns C, 2C, .. < n
inline size_t ckpt_bytes_h(const Layout& L, uint32_t n, size_t H, uint32_t C) {  // row 0 included
    return round_up(ckpt_cols_of(n, C) * (H + 1) * L.ck_row_bytes, L.ck_align);
}
inline size_t ckpt_bytes_of(const Layout& L, uint32_t n, uint32_t m, uint32_t C) { return ckpt_bytes_h(L, n, rows_of(L, m), C); }
inline size_t rowck_bytes_of(const Layout& L, uint32_t n, uint32_t m) { return (strips_of(L, m) - 1) * ((size_t)n + 1) * L.bnd_bytes; }
inline size_t tile_rows_of(const Layout& L, uint32_t m) { return std::min(rows_of(L, m), strip_rows(L)); }
inline size_t tile_cols_of(uint32_t n, uint32_t C) { return (size_t)std::min(n, C) + 1; }  // columns of the widest tile (column tile 0 has column 0 too)
inline size_t tile_bytes_h(const Layout& L, uint32_t n, size_t H, uint32_t C) { return round_up(tile_cols_of(n, C) * (std::min(H, strip_rows(L)) + 1), 16); }
inline size_t tile_bytes_of(const Layout& L, uint32_t n, uint32_t m, uint32_t C) { return tile_bytes_h(L, n, rows_of(L, m), C); }
// Device bytes of one pair: row checkpoints, column checkpoints, one tile of codes, the ops.
inline size_t tiled_bytes_of(const Layout& L, uint32_t n, uint32_t m, uint32_t C) {
    return rowck_bytes_of(L, n, m) + ckpt_bytes_of(L, n, m, C) + tile_bytes_of(L, n, m, C) + (size_t)n + m;
}
// Tiles a monotone path can visit: one more column tile or one more row tile per move.
inline uint32_t tile_visits_max(const Layout& L, uint32_t n, uint32_t m, uint32_t C) {
    return (uint32_t)((n + (size_t)C - 1) / C + (std::max<uint32_t>(m, 1) + strip_rows(L) - 1) / strip_rows(L));
}

// The planner's order: packed pairs by (g, |a|), then strip pairs by |a|; ties keep the order given.
inline std::vector<uint32_t> planner_order(const Layout& L, const std::vector<uint32_t>& n, const std::vector<uint32_t>& m) {
    std::vector<uint32_t> order(n.size());
    for (size_t p = 0; p < order.size(); ++p) order[p] = (uint32_t)p;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const int gx = packed(L, m[x]) ? seg_lg(L, m[x]) : 7, gy = packed(L, m[y]) ? seg_lg(L, m[y]) : 7;
        return gx != gy ? gx < gy : n[x] < n[y];
    });
    return order;
}

// The next chunk of a traced call: the pairs order[c0 .. c1), as many as fit the budget by size_of(pair) and at least one; *bytes is
// their sum.
template <class SizeOf>
std::vector<uint32_t> next_chunk(const std::vector<uint32_t>& order, size_t c0, size_t budget, SizeOf size_of, size_t* bytes) {
    size_t c1 = c0;
    *bytes = 0;
    while (c1 < order.size() && (c1 == c0 || *bytes + size_of(order[c1]) <= budget)) *bytes += size_of(order[c1]), ++c1;
    return std::vector<uint32_t>(order.begin() + c0, order.begin() + c1);
}

// What a pair keeps at Pair::codes during a launch: nothing (costs only), its traceback codes, or its column checkpoints -- the
// checkpoint pass of the tiled traceback, which also keeps a boundary row of every strip but the last instead of one per wave.
enum class Keep { kNone, kCodes, kCkpt };

struct PairSlot {
    uint32_t id;      // the pair
    uint32_t H, lg;   // rows_of(|b|) and the segment width of its wave (6 for a strip pair)
    size_t data_off;  // bytes into the code / column-checkpoint allocation (0 under kNone)
    size_t ops_off;   // bytes into the allocation of the walks' ops, |a| + |b| a pair (kCodes, kCkpt)
    size_t tile_off;  // bytes into the allocation of the tiles (kCkpt)
};
struct WaveSlot {
    uint32_t first, np, lg, strips, nmax;  // slots [first, first + np), all of segment width 1 << lg; the longest a
    size_t bnd_off;                        // strips > 1: bytes into the boundary-row allocation, else SIZE_MAX
};
// One launch's worth of waves over a subset of the pairs.
struct Waves {
    std::vector<WaveSlot> waves;  // most expensive first
    std::vector<PairSlot> pairs;  // in the order given
    size_t data_bytes = 0, ops_bytes = 0, tile_bytes = 0;
    size_t bnd_vals = 0;  // boundary values, Layout::bnd_bytes each
    double lanes = 0, slots = 0;
    size_t packed = 0, strip = 0;
};

// Waves over `ids` (in planner order): 64 / g packed pairs of one width per wave, a wave per strip pair; then most expensive first,
// by strips (nmax + g).
inline Waves plan_waves(const Layout& L, const std::vector<uint32_t>& n, const std::vector<uint32_t>& m, const std::vector<uint32_t>& ids, Keep keep,
                        uint32_t tile_cols = 0) {
    Waves P;
    P.pairs.reserve(ids.size());
    for (size_t x = 0; x < ids.size();) {
        const uint32_t p0 = ids[x];
        const bool pk = packed(L, m[p0]);
        const int lg = pk ? seg_lg(L, m[p0]) : 6;
        const size_t per = pk ? size_t(64) >> lg : 1;
        WaveSlot W{(uint32_t)P.pairs.size(), 0, (uint32_t)lg, (uint32_t)strips_of(L, m[p0]), 0, SIZE_MAX};
        const size_t H = pk ? size_t(L.rows) << lg : W.strips * strip_rows(L);  // of every pair of the wave
        while (x < ids.size() && W.np < per) {
            const uint32_t p = ids[x];
            if (packed(L, m[p]) != pk || (pk && seg_lg(L, m[p]) != lg)) break;
            ++x;
            P.pairs.push_back(PairSlot{p, (uint32_t)H, (uint32_t)lg, P.data_bytes, P.ops_bytes, P.tile_bytes});
            if (keep != Keep::kNone) P.ops_bytes += (size_t)n[p] + m[p];
            if (keep == Keep::kCodes) P.data_bytes += code_bytes_h(n[p], H);
            if (keep == Keep::kCkpt) {
                P.data_bytes += ckpt_bytes_h(L, n[p], H, tile_cols);
                P.tile_bytes += tile_bytes_h(L, n[p], H, tile_cols);
            }
            P.lanes += (double)((std::max<uint32_t>(m[p], 1) + L.rows - 1) / L.rows);
            W.nmax = std::max(W.nmax, n[p]);
            ++W.np;
            (pk ? P.packed : P.strip) += 1;
        }
        P.slots += 64.0 * W.strips;
        if (W.strips > 1) {  // a lone pair: nmax = n
            W.bnd_off = P.bnd_vals * L.bnd_bytes;
            P.bnd_vals += (keep == Keep::kCkpt ? size_t(W.strips) - 1 : 1) * ((size_t)W.nmax + 1);
        }
        P.waves.push_back(W);
    }
    std::stable_sort(P.waves.begin(), P.waves.end(), [](const WaveSlot& x, const WaveSlot& y) {
        return (uint64_t)x.strips * (x.nmax + (1u << x.lg)) > (uint64_t)y.strips * (y.nmax + (1u << y.lg));
    });
    return P;
}

// The tile job of a walk that stands at (i, j), not (0, 0), in a pair of |a| = n, |b| = m with column checkpoints C apart.  Row tile rt
// is 0 for j = 0, else the strip that owns row j; column tile ct is 0 for i = 0, else (i - 1) / C.  The job fills the rows of strip rt
// over the columns cs .. c1 = i, where c0 = ct C and cs = c0 + 1 (0 for c0 = 0: column 0 is a border of column tile 0); only lanes
// 0 .. rlast, the lane of row j, have to finish.
struct TileGeom {
    uint32_t ct, rt, c0, c1, Ht, row0, rlast, cols, steps;
    uint32_t lg;  // the job's segment width, 6 for a strip pair
    bool packed;
    // bytes into the pair's column checkpoints (ct > 0): the strip's rows of the checkpoint at c0, and its row 0
    size_t left_off, left0_off;
    size_t above_off;  // bytes into the pair's row checkpoints (rt > 0): the row of strip rt - 1
    double refill_cells;
};
// By the pair's H = rows_of(|b|) and its segment width, which the plan has (PairSlot); a packed pair is one with H <= 64 rows.
inline TileGeom tile_geom(const Layout& L, uint32_t n, size_t H, uint32_t lg, uint32_t C, uint32_t i, uint32_t j) {
    const uint32_t S = (uint32_t)strip_rows(L);
    TileGeom G{};
    G.packed = H <= S;
    G.lg = lg;
    G.ct = i ? (i - 1) / C : 0;
    G.rt = j ? (j - 1) / S : 0;
    G.c0 = G.ct * C;
    G.c1 = i;
    G.Ht = (uint32_t)std::min<size_t>(H, S);
    G.row0 = (uint32_t)(tile_cols_of(n, C) * G.Ht);
    G.rlast = j ? (j - 1 - G.rt * S) / L.rows : 0;
    G.cols = G.c1 - (G.c0 ? G.c0 + 1 : 0) + 1;
    G.steps = G.cols + G.rlast;
    if (G.ct) {
        G.left_off = ((size_t)(G.ct - 1) * H + (size_t)G.rt * S) * L.ck_row_bytes;
        G.left0_off = (ckpt_cols_of(n, C) * H + (G.ct - 1)) * L.ck_row_bytes;
    }
    if (G.rt) G.above_off = (size_t)(G.rt - 1) * ((size_t)n + 1) * L.bnd_bytes;
    G.refill_cells = (double)G.cols * L.rows * (G.rlast + 1);
    return G;
}
inline TileGeom tile_geom(const Layout& L, uint32_t n, uint32_t m, uint32_t C, uint32_t i, uint32_t j) {
    return tile_geom(L, n, rows_of(L, m), packed(L, m) ? (uint32_t)seg_lg(L, m) : 6, C, i, j);
}
// Tile jobs are grouped into waves like the planner's: a job joins the wave before it (np jobs of width 1 << lg so far) when both are
// packed pairs of one width and the wave is not full.
inline bool joins_tile_wave(const TileGeom& G, uint32_t lg, uint32_t np) { return G.packed && lg == G.lg && np < (64u >> lg); }

}  // namespace affine_plan
}  // namespace pa
