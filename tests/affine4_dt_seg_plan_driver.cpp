// Stand-alone check of csrc/affine4_dt_seg_plan.hpp (tests/test_affine4_dt_seg_plan.py builds it with the address and
// undefined-behaviour sanitizers and runs it): seeded random batches under five cost models against the properties the kernels of the
// segmented double-affine diagonal-transition traceback rely on.  Exit status 0 and "ok <batches> <chunks> <reads> <checkpoints>" when
// every property held, else the first violation on stderr and status 1.  What the header computes with formulas is restated here with
// loops, and every row index goes through the functions the kernels call.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "affine4_dt_seg_plan.hpp"

using namespace pa::affine4::dt;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::fprintf(stderr, "batch %d: ", batch);    \
            std::fprintf(stderr, __VA_ARGS__);            \
            std::fprintf(stderr, " (%s)\n", #cond);       \
            return 1;                                     \
        }                                                 \
    } while (0)

namespace {

const Costs kModels[5] = {
    {4, kAbsent, kAbsent, {6, 6, 24, 24}, {2, 2, 1, 1}},      // double_affine(4, 6, 2, 24, 1)
    {5, kAbsent, kAbsent, {3, 7, 15, 20}, {3, 2, 1, 1}},      // asymmetric
    {3, 5, 4, {4, 3, 12, 14}, {2, 2, 1, 1}},                  // linear edges too
    {2, kAbsent, kAbsent, {1, 1, 2, 2}, {9, 9, 8, 8}},        // steep: every extend above every open and the substitution
    {4, kAbsent, 900, {6, 1000, 1000, 7}, {2, 1000, 3, 1}},   // costs at the model's limit
};

// Where row `row` of a segment buffer stands: ring r's head (0), its body (1), the kNeg row (2), or nowhere (-1); *x: the front's
// cost it holds.
int locate(const SegRows& G, uint32_t S, int32_t s0, uint32_t row, int r, long long* x) {
    if (row == G.H + 5 * S) return 2;
    uint32_t base = 0;
    for (int q = 0; q < r; ++q) base += G.h[q] + S;
    if (row < base || row >= base + G.h[r] + S) return -1;
    *x = (long long)s0 - G.h[r] + (row - base);
    return row < base + G.h[r] ? 0 : 1;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20250612);
    const int batches = 300;
    size_t chunks_seen = 0, reads = 0, cks = 0, refused_batches = 0, multi_seg = 0, one_seg = 0;
    {
        const int batch = -1;  // the pinned sizes
        const SegRows G = seg_rows(kModels[0]);
        CHECK(G.h[0] == 24 && G.h[1] == 2 && G.h[2] == 2 && G.h[3] == 1 && G.h[4] == 1 && G.H == 30 && G.Ew == 24, "H %u Ew %u", G.H, G.Ew);
        CHECK(G.hoff[0] == 0 && G.hoff[1] == 24 && G.hoff[2] == 26 && G.hoff[3] == 28 && G.hoff[4] == 29, "hoff");
        const SegRows T = seg_rows(kModels[3]);
        CHECK(T.h[0] == 2 && T.H == 36 && T.Ew == 9, "steep: E %u H %u Ew %u", T.h[0], T.H, T.Ew);
        const SegRows B = seg_rows(kModels[4]);
        CHECK(B.h[0] == 1000 && B.H == 2006 && B.Ew == 1000, "heavy: E %u H %u Ew %u", B.h[0], B.H, B.Ew);
        // 3447 x 30 / 5 = 20682: 143^2 < 20682 <= 144^2; 24 segments; 36 + 23 x 30 + (30 + 720 + 1) = 1477 rows
        CHECK(seg_length(3446, G, 0) == 144 && seg_length(3455, G, 0) == 144 && seg_length(3456, G, 0) == 145, "default seg %u", seg_length(3446, G, 0));
        CHECK(seg_length(0, G, 0) == 24 && seg_length(10, G, 1000) == 24 && seg_length(30, G, 1000) == 31 && seg_length(145, T, 0) == 33, "seg");
        const SegShape S = seg_shape_of(10000, 10000, kModels[0], 3446, 0, false, false);
        const size_t row = (size_t)S.ring.W * 4;
        CHECK(S.ring.s_max == 3446 && S.S == 144 && S.nseg == 24, "S %u nseg %u", S.S, S.nseg);
        CHECK(S.ring_bytes == 36 * row && S.ck_bytes == 23 * 30 * row && S.buf_bytes == 751 * row && S.ops_bytes == 20000, "bytes");
        CHECK(S.bytes == 1477 * row + 20000 + 40, "%zu bytes", S.bytes);
        CHECK(ceil_sqrt(0) == 0 && ceil_sqrt(1) == 1 && ceil_sqrt(2) == 2 && ceil_sqrt(16) == 4 && ceil_sqrt(17) == 5, "ceil_sqrt");
        CHECK(ceil_sqrt((uint64_t)1 << 62) == (1u << 31), "ceil_sqrt at 2^62");
    }
    for (int batch = 0; batch < batches; ++batch) {
        const Costs& C = kModels[batch % 5];
        const bool fs = (batch / 5) % 2, fe = (batch / 10) % 2;
        // E, Ew and H by loops
        uint32_t E = 0, Ew = 0, H = 0;
        for (const uint32_t c : {C.sub, C.ins, C.del, C.open[0], C.open[1], C.open[2], C.open[3]})
            if (c != kAbsent) E = std::max(E, c);
        Ew = E, H = E;
        for (int t = 0; t < 4; ++t) Ew = std::max(Ew, C.ext[t]), H += C.ext[t];
        const SegRows G = seg_rows(C);
        CHECK(G.h[0] == E && G.Ew == Ew && G.H == H, "E %u Ew %u H %u", G.h[0], G.Ew, G.H);
        for (int t = 0; t < 4; ++t) CHECK(G.h[1 + t] == C.ext[t], "h of ring %d", 1 + t);
        const size_t np = 1 + rng() % 24;
        std::vector<uint32_t> n(np), m(np);
        for (size_t p = 0; p < np; ++p) {
            const uint32_t top = rng() % 6 == 0 ? 3000 : 300;
            n[p] = (uint32_t)(rng() % (top + 1));
            m[p] = rng() % 4 == 0 ? n[p] : (uint32_t)(rng() % (top + 1));
            if (rng() % 10 == 0) (rng() % 2 ? n[p] : m[p]) = 0;
        }
        int32_t s_max;
        switch (rng() % 4) {
            case 0: s_max = 0; break;
            case 1: s_max = (int32_t)(rng() % 60); break;
            case 2: s_max = (int32_t)(rng() % 4000); break;
            default: s_max = (1 << 30) - 1; break;
        }
        uint32_t seg;
        switch (rng() % 5) {
            case 0: seg = Ew; break;
            case 1: seg = Ew + 1; break;
            case 2: seg = Ew + (uint32_t)(rng() % (3 * Ew)); break;
            case 3: seg = (1u << 30) - 1; break;
            default: seg = 0; break;
        }
        std::vector<size_t> want_bytes(np);
        size_t total = 0, biggest = 0;
        for (size_t p = 0; p < np; ++p) {
            const SegShape sh = seg_shape_of(n[p], m[p], C, s_max, seg, fs, fe);
            const Shape ring = shape_of(n[p], m[p], C, s_max, false, fs, fe);
            CHECK(sh.ring.s_max == ring.s_max && sh.ring.W == ring.W && sh.ring.kmin == ring.kmin && sh.ring.kmax == ring.kmax && sh.ring.rows == ring.rows,
                  "pair %zu: the ring shape", p);
            const uint32_t sb = (uint32_t)ring.s_max;
            // S as stated: seg, or the smallest S with 5 S^2 >= (s' + 1) H raised to Ew; a length above max(Ew, s' + 1) is that
            uint32_t S = seg;
            if (!seg) {
                S = Ew;
                while (5 * (uint64_t)S * S < ((uint64_t)sb + 1) * H) ++S;
            }
            S = std::min(S, std::max(Ew, sb + 1));
            CHECK(sh.S == S && S >= Ew, "pair %zu: S = %u, expected %u", p, sh.S, S);
            CHECK(sh.nseg == sb / S + 1, "pair %zu: nseg %u", p, sh.nseg);
            (sh.nseg > 1 ? multi_seg : one_seg) += 1;
            // the byte formula
            const size_t row = (size_t)ring.W * 4;
            size_t ring_rows = (E + 1) + 1;
            for (int t = 0; t < 4; ++t) ring_rows += C.ext[t] + 1;
            CHECK(sh.ring_bytes == ring_rows * row && sh.ck_bytes == (size_t)(sh.nseg - 1) * H * row && sh.buf_bytes == ((size_t)H + 5 * (size_t)S + 1) * row,
                  "pair %zu: the regions", p);
            CHECK(sh.ops_bytes == (((size_t)n[p] + m[p] + 15) / 16) * 16, "pair %zu: ops", p);
            want_bytes[p] = sh.ring_bytes + sh.ck_bytes + sh.buf_bytes + sh.ops_bytes + 40;
            CHECK(sh.bytes == want_bytes[p], "pair %zu: %zu bytes, expected %zu", p, sh.bytes, want_bytes[p]);
            total += want_bytes[p];
            biggest = std::max(biggest, want_bytes[p]);
            if (p >= 2) continue;
            // every read s - c of the recurrence and of the walk, s in a segment, lands in that ring's head or body on the row of that
            // very front, or on the kNeg row; over the lowest two and the highest two segments
            const uint32_t bufrows = H + 5 * S + 1;
            CHECK(seg_neg_row(G, S) == bufrows - 1, "the kNeg row");
            for (uint32_t c = 0; c < sh.nseg; ++c) {
                if (c >= 2 && c + 2 < sh.nseg) continue;
                const int32_t s0 = (int32_t)(c * S);
                const int32_t s1 = (int32_t)std::min<uint64_t>((uint64_t)s0 + S - 1, sb);
                const int32_t step = S > 64 ? (int32_t)(S / 16) : 1;
                for (int32_t s = s0; s <= s1; s = (s + step > s1 && s != s1) ? s1 : s + step) {
                    // the front's own rows
                    for (int r = 0; r < 5; ++r) {
                        long long x = -1;
                        CHECK(locate(G, S, s0, seg_row(G, S, r, s0, s), r, &x) == 1 && x == s, "pair %zu: front %d of ring %d is stored at %lld", p, s, r, x);
                    }
                    // ring 0 at s - {sub, ins, del, open_t} (the step and the walk, on the main layer and inside a layer);
                    // ring 1 + t at s - e_t (extend, close, and the walk's step inside the layer)
                    for (int q = 0; q < 11; ++q) {
                        const int r = q < 7 ? 0 : q - 6;
                        const uint32_t cst = q == 0 ? C.sub : q == 1 ? C.ins : q == 2 ? C.del : q < 7 ? C.open[q - 3] : C.ext[q - 7];
                        ++reads;
                        if ((uint32_t)s < cst) continue;  // the kernels read the kNeg row
                        const uint32_t row = seg_row(G, S, r, s0, s - (int32_t)cst);
                        long long x = -1;
                        const int where = locate(G, S, s0, row, r, &x);
                        CHECK(row < bufrows - 1 && (where == 0 || where == 1) && x == (long long)s - cst,
                              "pair %zu: front %d - %u of ring %d reads row %u (%d, front %lld)", p, s, cst, r, row, where, x);
                        CHECK(where == 1 || c > 0, "pair %zu: segment 0 reads its head", p);
                    }
                }
            }
            // the forward pass: checkpoint rows are within the pair's rows and distinct, and boundary c holds for ring r exactly the
            // fronts cS - h_r .. cS - 1, at the rows the fill copies to the head of ring r
            const uint32_t nck = sh.nseg - 1;
            if ((uint64_t)nck * H <= 200000 && sb <= 300000) {
                std::set<uint32_t> rows;
                std::vector<size_t> per(5, 0);
                uint32_t sq = 0, sr = 0;
                for (uint32_t s = 0; s <= sb; ++s) {
                    for (int r = 0; r < 5; ++r) {
                        const bool want = s / S < nck && s % S + G.h[r] >= S;
                        CHECK(ck_takes(G, S, nck, r, sq, sr) == want, "pair %zu: front %u of ring %d", p, s, r);
                        if (!want) continue;
                        const uint32_t row = ck_row(G, S, r, sq, sr);
                        CHECK((uint64_t)row < (uint64_t)nck * H, "pair %zu: checkpoint row %u of %u", p, row, nck * H);
                        CHECK(rows.insert(row).second, "pair %zu: checkpoint row %u twice", p, row);
                        // the fill copies rows [hoff_r, hoff_r + h_r) of boundary sq to rows seg_base .. of the buffer
                        const int32_t s0 = (int32_t)((sq + 1) * S);
                        const uint32_t inhead = row - sq * H - G.hoff[r];
                        CHECK(row >= sq * H + G.hoff[r] && inhead < G.h[r], "pair %zu: checkpoint row %u is not of ring %d", p, row, r);
                        CHECK(seg_base(G, S, r) + inhead == seg_row(G, S, r, s0, (int32_t)s), "pair %zu: front %u of ring %d lands at head row %u", p, s, r,
                              inhead);
                        ++per[(size_t)r];
                        ++cks;
                    }
                    if (++sr == S) sr = 0, ++sq;
                }
                for (int r = 0; r < 5; ++r) CHECK(per[(size_t)r] == (size_t)nck * G.h[r], "pair %zu: %zu checkpoints of ring %d", p, per[(size_t)r], r);
                CHECK(rows.size() == (size_t)nck * H, "pair %zu: %zu checkpoint rows", p, rows.size());
            }
        }
        size_t budget;
        switch (batch % 4) {
            case 0: budget = total + 64; break;
            case 1: budget = biggest; break;
            case 2: budget = std::max(biggest, total / (2 + rng() % 6)); break;
            default: budget = biggest > 8 ? biggest - 1 - rng() % 8 : biggest; break;
        }
        const SegPlan P = seg_plan(n.data(), m.data(), np, C, s_max, seg, fs, fe, budget);
        long long over = -1;
        for (size_t p = 0; p < np && over < 0; ++p)
            if (want_bytes[p] > budget) over = (long long)p;
        CHECK(P.refused == over, "refused %lld, expected %lld at budget %zu", P.refused, over, budget);
        if (over >= 0) {
            ++refused_batches;
            CHECK(P.chunks.empty(), "a refused plan holds chunks");
            continue;
        }
        CHECK(P.shape.size() == np && P.order.size() == np && P.off.size() == np, "sizes");
        std::vector<int> seen(np, 0);
        for (size_t x = 0; x < np; ++x) {
            CHECK(P.order[x] < np && !seen[P.order[x]]++, "pair %u twice in the order", P.order[x]);
            if (x) {
                const Shape &A = P.shape[P.order[x - 1]].ring, &B = P.shape[P.order[x]].ring;
                CHECK(((uint64_t)A.s_max + 1) * A.W >= ((uint64_t)B.s_max + 1) * B.W, "order at %zu", x);
            }
        }
        size_t next = 0;
        for (const Chunk& c : P.chunks) {
            CHECK(c.count > 0 && c.first == next, "chunk at %zu", c.first);
            CHECK(c.bytes <= budget, "chunk of %zu bytes over the budget %zu", c.bytes, budget);
            const size_t fronts = c.bytes - c.count * kSegPairState;
            std::vector<std::pair<size_t, size_t>> span;  // [begin, end) of every region of every pair
            double wsum = 0;
            size_t sum = 0;
            for (size_t x = c.first; x < c.first + c.count; ++x) {
                const uint32_t p = P.order[x];
                const SegShape& sh = P.shape[p];
                size_t at = P.off[p];
                for (const size_t len : {sh.ring_bytes, sh.ck_bytes, sh.buf_bytes, sh.ops_bytes}) {
                    CHECK(at % 4 == 0, "pair %u: a region at offset %zu", p, at);
                    if (len) span.push_back({at, at + len});
                    at += len;
                }
                CHECK(at <= fronts, "pair %u ends at %zu of %zu", p, at, fronts);
                CHECK(sh.ops_bytes >= (size_t)n[p] + m[p], "pair %u: ops of %zu bytes", p, sh.ops_bytes);
                wsum += sh.ring.W;
                sum += sh.bytes;
            }
            CHECK(sum == c.bytes, "chunk of %zu bytes holds %zu", c.bytes, sum);
            std::sort(span.begin(), span.end());
            for (size_t x = 1; x < span.size(); ++x) CHECK(span[x - 1].second <= span[x].first, "regions overlap at %zu", span[x].first);
            CHECK(c.wide == (wsum / (double)c.count > 256.0), "wide = %d at a mean W of %f", (int)c.wide, wsum / (double)c.count);
            if (c.first + c.count < np) CHECK(c.bytes + P.shape[P.order[c.first + c.count]].bytes > budget, "chunk at %zu closed early", c.first);
            next += c.count;
            ++chunks_seen;
        }
        CHECK(next == np, "%zu pairs in chunks", next);
    }
    if (refused_batches == 0 || multi_seg == 0 || one_seg == 0) {
        std::fprintf(stderr, "%zu refused batches, %zu pairs of several segments and %zu of one: the batches miss a case\n", refused_batches, multi_seg, one_seg);
        return 1;
    }
    std::printf("ok %d %zu %zu %zu\n", batches, chunks_seen, reads, cks);
    return 0;
}
