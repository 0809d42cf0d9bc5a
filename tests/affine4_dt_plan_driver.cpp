// Stand-alone check of csrc/affine4_dt_plan.hpp (tests/test_affine4_dt_plan.py builds it with the address and undefined-behaviour
// sanitizers and runs it): seeded random batches under four cost models against the properties the double-affine diagonal-transition
// kernel relies on.  Exit status 0 and "ok <batches> <chunks> <reads>" when every property held, else the first violation on stderr and
// status 1.  What the header computes with divisions and formulas is restated here with loops.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "affine4_dt_plan.hpp"

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

const Costs kModels[4] = {
    {4, kAbsent, kAbsent, {6, 6, 24, 24}, {2, 2, 1, 1}},      // double_affine(4, 6, 2, 24, 1)
    {5, kAbsent, kAbsent, {3, 7, 15, 20}, {3, 2, 1, 1}},      // asymmetric
    {3, 5, 4, {4, 3, 12, 14}, {2, 2, 1, 1}},                  // linear edges too
    {4, kAbsent, 900, {6, 1000, 1000, 7}, {2, 1000, 3, 1}},   // costs at the model's limit
};

// The cheapest gap of length L, and the longest gap that s pays for, by trying every length.
uint64_t gap_slow(uint64_t L, uint32_t lin, const Costs& C, int t0) {
    if (L == 0) return 0;
    uint64_t c = std::min((uint64_t)C.open[t0] + L * C.ext[t0], (uint64_t)C.open[t0 + 2] + L * C.ext[t0 + 2]);
    if (lin != kAbsent) c = std::min<uint64_t>(c, L * lin);
    return c;
}
// (inside a layer the gap is `extend` short of closing: open + (L - 1) extend <= s)
uint32_t reach_slow(uint64_t s, uint32_t lin, const Costs& C, int t0, uint32_t cap) {
    uint32_t best = 0;
    for (uint32_t L = 1; L <= cap; ++L) {
        const bool lin_ok = lin != kAbsent && (uint64_t)L * lin <= s;
        const bool p0 = (uint64_t)C.open[t0] + (uint64_t)(L - 1) * C.ext[t0] <= s;
        const bool p1 = (uint64_t)C.open[t0 + 2] + (uint64_t)(L - 1) * C.ext[t0 + 2] <= s;
        if (!(lin_ok || p0 || p1)) break;  // (every price grows with L)
        best = L;
    }
    return best;
}

struct RingSim {
    uint32_t depth;
    int slot = 0;
    std::vector<long long> holds;  // which front a slot holds, -1: none
    explicit RingSim(uint32_t d) : depth(d), holds(d, -1) {}
    // the kernel's index: slot - c, wrapped once
    long long read(long long s, uint32_t c) const {
        if ((uint64_t)s < c) return -2;  // the kNeg row
        int x = slot - (int)c;
        x = x < 0 ? x + (int)depth : x;
        if (x < 0 || x >= (int)depth) return -3;
        return holds[(size_t)x];
    }
    void write(long long s) {
        holds[(size_t)slot] = s;
        slot = slot + 1 == (int)depth ? 0 : slot + 1;
    }
};

}  // namespace

int main() {
    std::mt19937_64 rng(20250311);
    const int batches = 320;
    size_t chunks_seen = 0, reads = 0, refused_batches = 0, wide_chunks = 0, narrow_chunks = 0;
    {
        const int batch = -1;  // the pinned sizes
        const Shape S = shape_of(10000, 10000, kModels[0], 1 << 20, false, false, false);
        CHECK(S.rows == 35 && S.depth[0] == 25 && S.depth[1] == 3 && S.depth[2] == 3 && S.depth[3] == 2 && S.depth[4] == 2, "rows %zu", S.rows);
        CHECK(S.s_max == 2 * (24 + 10000) && S.kmin == -10000 && S.kmax == 10000 && S.W == 20003, "s' %d W %u", S.s_max, S.W);
        CHECK(S.bytes == (size_t)36 * 20003 * 4 && S.ops_bytes == 0, "%zu bytes", S.bytes);
        const Shape T = shape_of(100, 60, kModels[0], 50, true, false, false);  // s' = 50: reach 27 on the second piece, 23 on the first
        CHECK(T.s_max == 50 && T.kmin == -27 && T.kmax == 27 && T.W == 57 && T.rows == 5 * 51, "traced: s' %d [%d, %d]", T.s_max, T.kmin, T.kmax);
        CHECK(T.ops_bytes == 160 && T.bytes == (size_t)(5 * 51 + 1) * 57 * 4 + 160, "traced: %zu bytes", T.bytes);
        const Shape B = shape_of(50, 50, kModels[3], 1 << 20, false, false, false);
        CHECK(B.depth[0] == 1001 && B.depth[1] == 3 && B.depth[2] == 1001 && B.depth[3] == 4 && B.depth[4] == 2, "open = 1000: main ring %u", B.depth[0]);
    }
    for (int batch = 0; batch < batches; ++batch) {
        const Costs& C = kModels[batch % 4];
        const bool traced = (batch / 4) % 2, fs = (batch / 8) % 2, fe = (batch / 16) % 2;
        const size_t np = 1 + rng() % 30;
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
            case 2: s_max = (int32_t)(rng() % 2000); break;
            default: s_max = (1 << 30) - 1; break;
        }
        if (traced && s_max > 4000) s_max = 4000;  // (the traced fronts of a loose bound are many megabytes: the budget below would refuse them all)
        // the expected shapes, by loops
        std::vector<size_t> want_bytes(np);
        size_t total = 0, biggest = 0;
        for (size_t p = 0; p < np; ++p) {
            const uint64_t always = (fs || fe ? 0 : gap_slow(n[p], C.del, C, 1)) + gap_slow(m[p], C.ins, C, 0);
            const int64_t sb = (int64_t)std::min<uint64_t>((uint64_t)s_max, always);
            const Shape S = shape_of(n[p], m[p], C, s_max, traced, fs, fe);
            CHECK(S.n == n[p] && S.m == m[p] && S.s_max == sb, "pair %zu: s' = %d, expected %lld", p, S.s_max, (long long)sb);
            // ring depths as stated
            uint32_t E = 0;
            for (const uint32_t c : {C.sub, C.ins, C.del, C.open[0], C.open[1], C.open[2], C.open[3]})
                if (c != kAbsent) E = std::max(E, c);
            CHECK(S.depth[0] == (traced ? (uint32_t)sb + 1 : E + 1), "pair %zu: main ring of %u", p, S.depth[0]);
            size_t rows = S.depth[0];
            for (int t = 0; t < 4; ++t) {
                CHECK(S.depth[t + 1] == (traced ? (uint32_t)sb + 1 : C.ext[t] + 1), "pair %zu: ring %d of %u", p, t, S.depth[t + 1]);
                rows += S.depth[t + 1];
            }
            CHECK(S.rows == rows, "pair %zu: %zu rows", p, S.rows);
            // the live range of every cost up to s' lies inside [kmin, kmax]
            const int64_t step = sb > 80 ? sb / 40 : 1;
            for (int64_t s = 0; s <= sb; s = (s + step > sb && s != sb) ? sb : s + step) {
                const int64_t klo = -(int64_t)std::min<uint32_t>(m[p], reach_slow((uint64_t)s, C.ins, C, 0, m[p]));
                const int64_t khi = (int64_t)std::min<uint32_t>(n[p], reach_slow((uint64_t)s, C.del, C, 1, n[p]));
                CHECK(klo >= S.kmin, "pair %zu: cost %lld reaches diagonal %lld below kmin %d", p, (long long)s, (long long)klo, S.kmin);
                if (!fs) CHECK(khi <= S.kmax, "pair %zu: cost %lld reaches diagonal %lld above kmax %d", p, (long long)s, (long long)khi, S.kmax);
            }
            const int64_t back = reach_slow((uint64_t)sb, C.ins, C, 0, m[p] + n[p] + 1);
            if (fs) {
                // every end diagonal a path within s' can come back to, and no more than |a|
                CHECK(S.kmax == std::min<int64_t>(n[p], std::max<int64_t>(0, (int64_t)n[p] - (int64_t)m[p] + back)), "pair %zu: kmax %d", p, S.kmax);
            } else {
                CHECK(S.kmax == (int64_t)std::min<uint32_t>(n[p], reach_slow((uint64_t)sb, C.del, C, 1, n[p])), "pair %zu: kmax %d is not tight", p, S.kmax);
            }
            CHECK(S.kmin == -(int64_t)std::min<int64_t>(m[p], back), "pair %zu: kmin %d is not tight", p, S.kmin);
            CHECK(S.kmin <= 0 && S.kmax >= 0 && S.kmax <= (int32_t)n[p] && -S.kmin <= (int32_t)m[p], "pair %zu: [%d, %d]", p, S.kmin, S.kmax);
            CHECK(S.W == (uint32_t)(S.kmax - S.kmin + 3), "pair %zu: W %u", p, S.W);
            CHECK(S.ops_bytes == (traced ? (((size_t)n[p] + m[p] + 15) / 16) * 16 : 0), "pair %zu: %zu bytes of ops", p, S.ops_bytes);
            want_bytes[p] = (rows + 1) * (size_t)S.W * 4 + S.ops_bytes;
            CHECK(S.bytes == want_bytes[p], "pair %zu: %zu bytes, expected %zu", p, S.bytes, want_bytes[p]);
            total += want_bytes[p];
            biggest = std::max(biggest, want_bytes[p]);
            // every read s - c of the recurrence finds its front: the slot was not written since (the cost-only rings; the traced ones
            // never wrap), up to a few wraps of the deepest ring
            if (!traced && p < 3) {
                RingSim R[5] = {RingSim(S.depth[0]), RingSim(S.depth[1]), RingSim(S.depth[2]), RingSim(S.depth[3]), RingSim(S.depth[4])};
                const int64_t upto = std::min<int64_t>(sb, 3 * (int64_t)S.depth[0] + 7);
                for (int64_t s = 0; s <= upto; ++s) {
                    for (const uint32_t c : {C.sub, C.ins, C.del, C.open[0], C.open[1], C.open[2], C.open[3]}) {
                        const long long got = R[0].read(s, c);
                        CHECK(got == ((uint64_t)s < c ? -2 : s - (long long)c), "pair %zu: front %lld - %u of the main ring reads %lld", p, (long long)s, c, got);
                        ++reads;
                    }
                    for (int t = 0; t < 4; ++t) {
                        const long long got = R[t + 1].read(s, C.ext[t]);
                        CHECK(got == ((uint64_t)s < C.ext[t] ? -2 : s - (long long)C.ext[t]), "pair %zu: front %lld - %u of ring %d reads %lld", p,
                              (long long)s, C.ext[t], t, got);
                        ++reads;
                    }
                    for (RingSim& r : R) r.write(s);
                }
            }
        }
        // budgets: everything in one chunk, exactly the biggest pair, a fraction of the total, a few bytes short of a pair (refusal)
        size_t budget;
        switch (batch % 5) {
            case 0: budget = total + 64; break;
            case 1: budget = biggest; break;
            case 2: budget = std::max(biggest, total / (2 + rng() % 6)); break;
            case 3: budget = std::max(biggest, total / 2 + 1); break;
            default: budget = biggest > 8 ? biggest - 1 - rng() % 8 : biggest; break;
        }
        const Plan P = plan(n.data(), m.data(), np, C, s_max, traced, fs, fe, budget);
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
        // the order is a permutation, most expensive first
        std::vector<int> seen(np, 0);
        for (size_t x = 0; x < np; ++x) {
            CHECK(P.order[x] < np && !seen[P.order[x]]++, "pair %u twice in the order", P.order[x]);
            if (x) {
                const Shape &A = P.shape[P.order[x - 1]], &B = P.shape[P.order[x]];
                CHECK(((uint64_t)A.s_max + 1) * A.W >= ((uint64_t)B.s_max + 1) * B.W, "order at %zu", x);
            }
        }
        // the chunks tile the order; each is within the budget; its pairs' buffers are disjoint and inside it
        size_t next = 0;
        for (const Chunk& c : P.chunks) {
            CHECK(c.count > 0 && c.first == next, "chunk at %zu", c.first);
            CHECK(c.bytes <= budget, "chunk of %zu bytes over the budget %zu", c.bytes, budget);
            std::vector<std::pair<size_t, size_t>> span;  // [begin, end) of every pair
            double wsum = 0;
            for (size_t x = c.first; x < c.first + c.count; ++x) {
                const uint32_t p = P.order[x];
                CHECK(P.off[p] % 4 == 0, "pair %u at offset %zu", p, P.off[p]);
                span.push_back({P.off[p], P.off[p] + P.shape[p].bytes});
                wsum += P.shape[p].W;
                // the ops stand behind the fronts, inside the pair's bytes
                CHECK(P.shape[p].bytes - P.shape[p].ops_bytes == (P.shape[p].rows + 1) * (size_t)P.shape[p].W * 4, "pair %u: fronts and ops overlap", p);
                CHECK(!traced || P.shape[p].ops_bytes >= (size_t)n[p] + m[p], "pair %u: ops of %zu bytes", p, P.shape[p].ops_bytes);
            }
            std::sort(span.begin(), span.end());
            for (size_t x = 0; x < span.size(); ++x) {
                CHECK(span[x].first < span[x].second || P.shape[P.order[c.first]].bytes == 0, "an empty span");
                CHECK(x == 0 || span[x - 1].second <= span[x].first, "pairs overlap at %zu", span[x].first);
            }
            CHECK(span.back().second <= c.bytes, "a pair ends at %zu of %zu", span.back().second, c.bytes);
            CHECK(c.wide == (wsum / (double)c.count > 256.0), "wide = %d at a mean W of %f", (int)c.wide, wsum / (double)c.count);
            // the chunk is full: the next pair did not fit
            if (c.first + c.count < np) CHECK(c.bytes + P.shape[P.order[c.first + c.count]].bytes > budget, "chunk at %zu closed early", c.first);
            (c.wide ? wide_chunks : narrow_chunks) += 1;
            next += c.count;
            ++chunks_seen;
        }
        CHECK(next == np, "%zu pairs in chunks", next);
    }
    if (refused_batches == 0 || wide_chunks == 0 || narrow_chunks == 0) {
        std::fprintf(stderr, "%zu refused batches, %zu wide and %zu narrow chunks: the batches miss a case\n", refused_batches, wide_chunks, narrow_chunks);
        return 1;
    }
    std::printf("ok %d %zu %zu\n", batches, chunks_seen, reads);
    return 0;
}
