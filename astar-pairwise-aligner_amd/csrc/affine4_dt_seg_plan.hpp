// affine4_dt_seg_plan.hpp -- the host geometry of the segmented traceback of the double-affine diagonal-transition route
// (affine4_dt_seg_unit.hip, affine4_dt_seg_kernel.hpp), plain C++ without HIP so that tests/affine4_dt_seg_plan_driver.cpp can check it
// under the sanitizers without a GPU.  The sibling of affine4_dt_plan.hpp, whose Costs, Shape and Chunk it uses.
//
// The argument.  With E = main_edge(C) and e_t = ext[t]: front s reads the main layer at s - {sub, ins, del, open_t} >= s - E and layer
// t at s - e_t only.  The walk reads the same fronts: on the main layer at s it reads main at s - c, c <= E, and layer t at s - e_t;
// inside layer t it reads main at s - open_t and layer t at s - e_t.  One walk step lowers s by at most Ew = max(E, e_0 .. e_3), which
// can exceed E: an extend may cost more than every open and every linear edge.  Cut the costs into segments of S >= Ew, segment c =
// [cS, cS + S - 1].  Recomputing and walking segment c needs, below cS, the last E fronts of the main layer and the last e_t of layer
// t: H = E + e_0 + e_1 + e_2 + e_3 rows, not 5 Ew; and the walk leaves segment c into segment c - 1, never past it.
//
// Rings: ring 0 is the main layer, ring 1 + t layer t; h_0 = E and h_{1+t} = e_t.
//   checkpoint rows  boundary c = 1 .. nseg - 1 holds H rows, ring after ring: front s of ring r, cS - h_r <= s < cS, is row
//                    (c - 1) H + hoff_r + s - (cS - h_r), hoff_r = h_0 + .. + h_{r-1}.
//   segment buffer   ring after ring, ring r being h_r head rows (fronts s0 - h_r .. s0 - 1) and then S rows (fronts s0 .. s0 + S - 1):
//                    front x of ring r is row base_r + h_r + x - s0, base_r = hoff_r + r S.  Row H + 5 S is the kNeg row, which a front
//                    below cost 0 or over an absent edge reads.
//
// Device bytes of a pair, all sized from its bound s' before anything runs, nseg = s' / S + 1, every row W x 4 bytes:
//   ring   (E + 1) + sum (e_t + 1) + 1 rows: the cost-only rings of affine4_dt_plan.hpp and their kNeg row
//   ck     (nseg - 1) H rows
//   buf    H + 5 S + 1 rows
//   ops    |a| + |b| rounded up to 16
//   state  kSegPairState bytes: the walk state and the fills' counters
// S is `seg`, or for seg = 0 the smallest S with 5 S^2 >= (s' + 1) H raised to Ew, which balances checkpoints against the segment
// buffer; either way a length above max(Ew, s' + 1) is that, one segment.
#pragma once
#include "affine4_dt_plan.hpp"

namespace pa {
namespace affine4 {
namespace dt {

constexpr uint64_t kSegRowsMax = uint64_t(1) << 31;  // rows of a segment buffer or of a pair's checkpoints: the kernels index rows in 32 bits
constexpr size_t kSegPairState = 40;  // sizeof(WalkState) + sizeof(Stat), which affine4_dt_seg_unit.hip asserts

// The rows below a segment, per ring; passed to the kernels by value.
struct SegRows {
    uint32_t h[5];     // E, e_0 .. e_3
    uint32_t hoff[5];  // h_0 + .. + h_{r-1}
    uint32_t H, Ew;
};

inline SegRows seg_rows(const Costs& C) {
    SegRows G{};
    G.h[0] = main_edge(C);
    for (int t = 0; t < 4; ++t) G.h[1 + t] = C.ext[t];
    for (int r = 0; r < 5; ++r) {
        G.hoff[r] = G.H;
        G.H += G.h[r];
        G.Ew = std::max(G.Ew, G.h[r]);
    }
    return G;
}

#if defined(__HIPCC__)
#define PA_SEG_HD __host__ __device__ inline
#else
#define PA_SEG_HD inline
#endif

// Row of front x of ring r in the buffer of the segment that starts at s0 (x >= s0 - h_r), and the buffer's kNeg row.  Rows are 32-bit:
// H + 5 S + 1 stays below 2^32 for every pair that runs, since seg_plan refuses a pair whose buffer has more rows than kSegRowsMax
// whatever the budget (under costs of at most 1000 such an S needs a bound, and so a W, of hundreds of thousands: petabytes).
PA_SEG_HD uint32_t seg_base(const SegRows& G, uint32_t S, int r) { return G.hoff[r] + (uint32_t)r * S; }
PA_SEG_HD uint32_t seg_row(const SegRows& G, uint32_t S, int r, int32_t s0, int32_t x) { return seg_base(G, S, r) + G.h[r] + (uint32_t)(x - s0); }
PA_SEG_HD uint32_t seg_neg_row(const SegRows& G, uint32_t S) { return G.H + 5 * S; }
// Whether the forward pass stores front s = sq S + sr of ring r to the checkpoint rows, and to which.
PA_SEG_HD bool ck_takes(const SegRows& G, uint32_t S, uint32_t nck, int r, uint32_t sq, uint32_t sr) { return sq < nck && sr + G.h[r] >= S; }
PA_SEG_HD uint32_t ck_row(const SegRows& G, uint32_t S, int r, uint32_t sq, uint32_t sr) { return sq * G.H + G.hoff[r] + (sr + G.h[r] - S); }

inline uint32_t ceil_sqrt(uint64_t x) {
    uint64_t r = 0;
    for (uint64_t bit = uint64_t(1) << 31; bit; bit >>= 1)
        if ((r + bit) * (r + bit) <= x) r += bit;
    return (uint32_t)(r * r == x ? r : r + 1);
}

// The segment length of a pair whose bound is `bound`.  seg: 0, or in [Ew, 2^30).
inline uint32_t seg_length(uint32_t bound, const SegRows& G, uint32_t seg) {
    uint32_t S = seg ? seg : std::max(G.Ew, ceil_sqrt((((uint64_t)bound + 1) * G.H + 4) / 5));
    return std::min(S, std::max(G.Ew, bound + 1));
}

struct SegShape {
    Shape ring;     // the cost-only shape: bound, diagonals, W, ring depths
    uint32_t S;     // costs of a segment
    uint32_t nseg;  // s' / S + 1: segments the bound reaches; nseg - 1 boundaries have checkpoint rows
    size_t ring_bytes, ck_bytes, buf_bytes, ops_bytes;
    size_t bytes;   // their sum and kSegPairState
};

inline SegShape seg_shape_of(uint32_t n, uint32_t m, const Costs& C, int32_t s_max, uint32_t seg, bool fs, bool fe) {
    SegShape sh{};
    const SegRows G = seg_rows(C);
    sh.ring = shape_of(n, m, C, s_max, false, fs, fe);
    const size_t row = (size_t)sh.ring.W * 4;
    sh.S = seg_length((uint32_t)sh.ring.s_max, G, seg);
    sh.nseg = (uint32_t)sh.ring.s_max / sh.S + 1;
    sh.ring_bytes = (sh.ring.rows + 1) * row;
    sh.ck_bytes = (size_t)(sh.nseg - 1) * G.H * row;
    sh.buf_bytes = ((size_t)G.H + 5 * (size_t)sh.S + 1) * row;
    sh.ops_bytes = ((size_t)n + m + 15) & ~size_t(15);
    sh.bytes = sh.ring_bytes + sh.ck_bytes + sh.buf_bytes + sh.ops_bytes + kSegPairState;
    return sh;
}

// The chunks of a batch: most expensive pair first (cost steps x diagonals), each chunk within the budget.  A pair's four regions
// (ring | checkpoints | segment buffer | ops) stand at off[p] of the chunk's fronts; the kSegPairState bytes of every pair stand in
// buffers of their own, indexed by the pair's place in the chunk, and count towards Chunk::bytes.
struct SegPlan {
    std::vector<SegShape> shape;
    std::vector<uint32_t> order;
    std::vector<size_t> off;
    std::vector<Chunk> chunks;
    long long refused = -1;  // the first pair whose bytes alone exceed the budget (or whose rows exceed kSegRowsMax): no chunks then
};

inline SegPlan seg_plan(const uint32_t* n, const uint32_t* m, size_t np, const Costs& C, int32_t s_max, uint32_t seg, bool fs, bool fe, size_t budget) {
    SegPlan P;
    P.shape.resize(np);
    for (size_t p = 0; p < np; ++p) {
        P.shape[p] = seg_shape_of(n[p], m[p], C, s_max, seg, fs, fe);
        const SegShape& sh = P.shape[p];
        const uint64_t H = seg_rows(C).H;
        if (sh.bytes > budget || H + 5 * (uint64_t)sh.S + 1 > kSegRowsMax || (uint64_t)(sh.nseg - 1) * H > kSegRowsMax) {
            P.refused = (long long)p;
            return P;
        }
    }
    P.order.resize(np);
    P.off.assign(np, 0);
    for (size_t p = 0; p < np; ++p) P.order[p] = (uint32_t)p;
    std::stable_sort(P.order.begin(), P.order.end(), [&](uint32_t x, uint32_t y) {
        return ((uint64_t)P.shape[x].ring.s_max + 1) * P.shape[x].ring.W > ((uint64_t)P.shape[y].ring.s_max + 1) * P.shape[y].ring.W;
    });
    for (size_t c0 = 0; c0 < np;) {
        size_t c1 = c0, total = 0, fronts = 0;
        double wsum = 0;
        while (c1 < np && (c1 == c0 || total + P.shape[P.order[c1]].bytes <= budget)) {
            const SegShape& sh = P.shape[P.order[c1]];
            P.off[P.order[c1]] = fronts;
            fronts += sh.bytes - kSegPairState;
            total += sh.bytes;
            wsum += sh.ring.W;
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
