// affine4_dt_plan.hpp -- the host geometry of the double-affine diagonal-transition route (affine4_dt_unit.hip), plain C++ without HIP so
// that tests/affine4_dt_plan_driver.cpp can check it under the sanitizers without a GPU, in the manner of affine_plan.hpp.
//
// From a pair's lengths, the cost record, s_max, the ends-free switches and traced / not: the pair's bound s', its diagonals
// [kmin, kmax] and row width W, the five ring depths, and its device bytes; from those the order and the chunks of a batch within a
// byte budget, most expensive pair first.
//
// Ring depths.  Front s reads the main layer at s - {sub, ins, del, open_0 .. open_3} and layer t at s - extend_t only (extend and
// close both cost extend_t).  So the main layer keeps E + 1 fronts, E the largest of those seven edges that the model has, and layer t
// keeps extend_t + 1, each ring with a slot counter of its own: under double_affine(4, 6, 2, 24, 1) that is 25 + 3 + 3 + 2 + 2 rows of W
// values and one never-written row for every front below 0, 36 in all, where (largest edge + 1) x 5 would be 130.  The traced call keeps
// every front: all five depths are s' + 1.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pa {
namespace affine4 {
namespace dt {

constexpr uint32_t kAbsent = 1u << 30;  // the cost of an edge the model does not have (sub, ins, del only: all four layers are required)
constexpr double kWideMean = 256;       // mean W of a chunk's pairs above which its blocks are kWideBlock threads wide

// The edge costs as diagonal transition sees them: opening layer t costs open[t] and consumes a byte, extending costs ext[t] and
// consumes one, closing costs ext[t] and consumes nothing.  Layers 0 and 2 insert (consume b), 1 and 3 delete (consume a).
struct Costs {
    uint32_t sub, ins, del;
    uint32_t open[4], ext[4];
};

inline uint64_t piece_cost(uint64_t L, uint32_t op, uint32_t ex) { return op + L * ex; }
// The cheapest way to pay one gap of length L: the linear edge, or either piece.
inline uint64_t gap_cost(uint64_t L, uint32_t lin, uint32_t o0, uint32_t e0, uint32_t o1, uint32_t e1) {
    if (L == 0) return 0;
    uint64_t c = std::min(piece_cost(L, o0, e0), piece_cost(L, o1, e1));
    if (lin != kAbsent) c = std::min<uint64_t>(c, L * lin);
    return c;
}
inline uint64_t ins_cost(uint64_t L, const Costs& C) { return gap_cost(L, C.ins, C.open[0], C.ext[0], C.open[2], C.ext[2]); }
inline uint64_t del_cost(uint64_t L, const Costs& C) { return gap_cost(L, C.del, C.open[1], C.ext[1], C.open[3], C.ext[3]); }

// The longest gap cost s pays for on any layer of one direction: s / lin on the main layer, (s - open) / extend + 1 inside a layer
// (which is `extend` short of closing).
inline uint32_t reach(uint32_t s, uint32_t lin, uint32_t o0, uint32_t e0, uint32_t o1, uint32_t e1) {
    uint32_t r = lin != kAbsent ? s / lin : 0;
    if (s >= o0) r = std::max(r, (s - o0) / e0 + 1);
    if (s >= o1) r = std::max(r, (s - o1) / e1 + 1);
    return r;
}
inline uint32_t reach_ins(uint32_t s, const Costs& C) { return reach(s, C.ins, C.open[0], C.ext[0], C.open[2], C.ext[2]); }
inline uint32_t reach_del(uint32_t s, const Costs& C) { return reach(s, C.del, C.open[1], C.ext[1], C.open[3], C.ext[3]); }

// E: the largest edge at which the main layer is read.
inline uint32_t main_edge(const Costs& C) {
    uint32_t e = std::max(std::max(C.open[0], C.open[1]), std::max(C.open[2], C.open[3]));
    for (const uint32_t c : {C.sub, C.ins, C.del})
        if (c != kAbsent) e = std::max(e, c);
    return e;
}

// One pair.  Row r of its fronts is W values; the rings stand one after the other, main first, and the kNeg row last.
struct Shape {
    uint32_t n, m;
    int32_t s_max;       // s': min(the call's s_max, the cost of the path that is always there)
    int32_t kmin, kmax;  // the live range at s'; diagonal k is column k - kmin + 1 of a row
    uint32_t W;          // kmax - kmin + 3: a padding column on either side
    uint32_t depth[5];   // slots of the main layer's ring and of layers 0 .. 3
    size_t rows;         // the sum of the depths (the kNeg row is row `rows`)
    size_t ops_bytes;    // traced: |a| + |b| rounded up to 16, behind the fronts
    size_t bytes;        // (rows + 1) W 4 + ops_bytes
};

// The path that is always there: deleting a and inserting b; with either end free inserting b (end = 0, or start = |a|).  Under
// free_start the diagonals up to kmax are live from cost 0 on, kmax = min(|a|, |a| - |b| + reach_ins(s')): a path through a diagonal
// above that needs more insertions than s' pays for to come back to an end diagonal (<= |a| - |b|), so the results are those of |a|.
inline Shape shape_of(uint32_t n, uint32_t m, const Costs& C, int32_t s_max, bool traced, bool fs, bool fe) {
    Shape S{};
    S.n = n;
    S.m = m;
    S.s_max = (int32_t)std::min<uint64_t>((uint64_t)s_max, (fs || fe ? 0 : del_cost(n, C)) + ins_cost(m, C));
    const uint32_t back = reach_ins((uint32_t)S.s_max, C);
    S.kmin = -(int32_t)std::min(m, back);
    S.kmax = fs ? (int32_t)std::min<int64_t>(n, std::max<int64_t>(0, (int64_t)n - (int64_t)m + back))
                : (int32_t)std::min(n, reach_del((uint32_t)S.s_max, C));
    S.W = (uint32_t)(S.kmax - S.kmin + 3);
    S.depth[0] = traced ? (uint32_t)S.s_max + 1 : main_edge(C) + 1;
    for (int t = 0; t < 4; ++t) S.depth[t + 1] = traced ? (uint32_t)S.s_max + 1 : C.ext[t] + 1;
    S.rows = 0;
    for (const uint32_t d : S.depth) S.rows += d;
    S.ops_bytes = traced ? (((size_t)n + m + 15) & ~size_t(15)) : 0;
    S.bytes = (S.rows + 1) * S.W * 4 + S.ops_bytes;
    return S;
}

struct Chunk {
    size_t first, count;  // order[first .. first + count)
    size_t bytes;
    bool wide;            // its blocks are kWideBlock threads
};

struct Plan {
    std::vector<Shape> shape;     // by pair
    std::vector<uint32_t> order;  // most expensive first: cost steps x diagonals
    std::vector<size_t> off;      // by pair: byte offset of its fronts in its chunk's allocation
    std::vector<Chunk> chunks;
    long long refused = -1;       // the first pair whose bytes alone exceed the budget: no chunks then
};

inline Plan plan(const uint32_t* n, const uint32_t* m, size_t np, const Costs& C, int32_t s_max, bool traced, bool fs, bool fe, size_t budget) {
    Plan P;
    P.shape.resize(np);
    for (size_t p = 0; p < np; ++p) {
        P.shape[p] = shape_of(n[p], m[p], C, s_max, traced, fs, fe);
        if (P.shape[p].bytes > budget) {
            P.refused = (long long)p;
            return P;
        }
    }
    P.order.resize(np);
    P.off.assign(np, 0);
    for (size_t p = 0; p < np; ++p) P.order[p] = (uint32_t)p;
    std::stable_sort(P.order.begin(), P.order.end(), [&](uint32_t x, uint32_t y) {
        return ((uint64_t)P.shape[x].s_max + 1) * P.shape[x].W > ((uint64_t)P.shape[y].s_max + 1) * P.shape[y].W;
    });
    for (size_t c0 = 0; c0 < np;) {
        size_t c1 = c0, total = 0;
        double wsum = 0;
        while (c1 < np && (c1 == c0 || total + P.shape[P.order[c1]].bytes <= budget)) {
            P.off[P.order[c1]] = total;
            total += P.shape[P.order[c1]].bytes;
            wsum += P.shape[P.order[c1]].W;
            ++c1;
        }
        P.chunks.push_back(Chunk{c0, c1 - c0, total, wsum / (double)(c1 - c0) > kWideMean});
        c0 = c1;
    }
    return P;
}

}  // namespace dt
}  // namespace affine4
}  // namespace pa
