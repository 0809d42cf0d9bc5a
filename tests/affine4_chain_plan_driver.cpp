// Stand-alone check of csrc/affine_chain_plan.hpp with 16-byte boundary values, as the double-affine batch plans its chained route
// (tests/test_affine4_chain_plan.py builds it with the address and undefined-behaviour sanitizers and runs it): seeded random batches
// against the properties the chained kernel relies on, and plan(pairs, B) against plan(pairs, B, 8).  Exit status 0 and "ok <batches>
// <refused>" when every property held, else the first violation on stderr and status 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "affine_chain_plan.hpp"

using namespace pa::affine_chain;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::fprintf(stderr, "batch %d: ", batch);    \
            std::fprintf(stderr, __VA_ARGS__);            \
            std::fprintf(stderr, " (%s)\n", #cond);       \
            return 1;                                     \
        }                                                 \
    } while (0)

constexpr size_t kValue = 16;  // {M, I1, I2, 0}

static bool same(const Plan& A, const Plan& B) {
    if (A.refused != B.refused || A.words_max != B.words_max || A.row_off != B.row_off || A.jobs.size() != B.jobs.size() || A.chunks.size() != B.chunks.size())
        return false;
    for (size_t j = 0; j < A.jobs.size(); ++j)
        if (A.jobs[j].pair != B.jobs[j].pair || A.jobs[j].strip != B.jobs[j].strip) return false;
    for (size_t c = 0; c < A.chunks.size(); ++c)
        if (A.chunks[c].first_pair != B.chunks[c].first_pair || A.chunks[c].npairs != B.chunks[c].npairs || A.chunks[c].first_job != B.chunks[c].first_job ||
            A.chunks[c].njobs != B.chunks[c].njobs || A.chunks[c].words != B.chunks[c].words)
            return false;
    return true;
}

int main() {
    std::mt19937_64 rng(20250311);
    int refused_batches = 0;
    const int batches = 400;
    for (int batch = 0; batch < batches; ++batch) {
        const size_t np = 1 + rng() % 40;
        std::vector<Shape> pairs(np);
        size_t total = 0, biggest = 0, jobs_want = 0;
        for (Shape& p : pairs) {
            p.m = 1025 + (uint32_t)(rng() % (40000 - 1025 + 1));
            p.n = (uint32_t)(rng() % 5001);
            if (rng() % 8 == 0) p.m = 1025 + (uint32_t)(rng() % 3) * 1023;  // 1025, 2048, 3071: the strip edges
            const size_t bytes = (((size_t)p.m + 1023) / 1024 - 1) * ((size_t)p.n + 1) * kValue;  // written out here, not taken from the header
            CHECK(pair_bytes(p, kValue) == bytes && pair_words(p, kValue) * kValue == bytes, "pair_bytes %zu, expected %zu", pair_bytes(p, kValue), bytes);
            total += bytes;
            biggest = std::max(biggest, bytes);
            jobs_want += ((size_t)p.m + 1023) / 1024;
        }
        // budgets: everything in one chunk, exactly the biggest pair, a fraction of the total, a few bytes short of a pair (refusal)
        size_t budget;
        switch (batch % 4) {
            case 0: budget = total + 64; break;
            case 1: budget = biggest; break;
            case 2: budget = std::max(biggest, total / (2 + rng() % 6)); break;
            default: budget = biggest > kValue ? biggest - 1 - rng() % kValue : biggest; break;
        }
        // the default value size is the two-layer batch's
        CHECK(same(plan(pairs, budget), plan(pairs, budget, 8)), "plan(pairs, B) differs from plan(pairs, B, 8) at budget %zu", budget);
        const Plan P = plan(pairs, budget, kValue);
        // a pair over budget is refused (the first such pair is named), and nothing else is refused
        long long over = -1;
        for (size_t p = 0; p < np && over < 0; ++p)
            if ((((size_t)pairs[p].m + 1023) / 1024 - 1) * ((size_t)pairs[p].n + 1) * kValue > budget) over = (long long)p;
        CHECK(P.refused == over, "refused %lld, expected %lld at budget %zu", P.refused, over, budget);
        if (over >= 0) {
            ++refused_batches;
            CHECK(P.jobs.empty() && P.chunks.empty(), "a refused plan holds jobs");
            continue;
        }
        CHECK(P.jobs.size() == jobs_want, "%zu jobs, expected %zu", P.jobs.size(), jobs_want);
        CHECK(P.row_off.size() == np, "row_off of %zu pairs", P.row_off.size());
        // chunks tile the pairs and the jobs in order
        size_t next_pair = 0, next_job = 0, words_max = 0;
        for (const Chunk& c : P.chunks) {
            CHECK(c.npairs > 0 && c.first_pair == next_pair && c.first_job == next_job, "chunk at pair %zu job %zu", c.first_pair, c.first_job);
            CHECK(c.words * kValue <= budget, "chunk of %zu bytes over the budget %zu", c.words * kValue, budget);
            words_max = std::max(words_max, c.words);
            // a pair's jobs are contiguous and ascending, and every job's producer is the job before it
            size_t j = c.first_job;
            std::vector<std::pair<size_t, size_t>> rows;  // [begin, end) of every (pair, strip) row in the chunk's allocation, in bytes
            for (size_t p = c.first_pair; p < c.first_pair + c.npairs; ++p) {
                const size_t S = ((size_t)pairs[p].m + 1023) / 1024, w = ((size_t)pairs[p].n + 1) * kValue;
                CHECK(S >= 2, "pair %zu has %zu strips", p, S);
                for (size_t s = 0; s < S; ++s, ++j) {
                    CHECK(j < c.first_job + c.njobs, "pair %zu strip %zu beyond the chunk's jobs", p, s);
                    CHECK(P.jobs[j].pair == p && P.jobs[j].strip == s, "job %zu is (%u, %u), expected (%zu, %zu)", j, P.jobs[j].pair, P.jobs[j].strip, p, s);
                    if (s > 0) CHECK(P.jobs[j - 1].pair == p && P.jobs[j - 1].strip == s - 1, "job %zu: its producer is not job %zu", j, j - 1);
                    if (s + 1 < S) {
                        const size_t b = P.row_off[p] * kValue + s * w;
                        CHECK(b + w <= c.words * kValue, "row of (%zu, %zu) ends at byte %zu of %zu", p, s, b + w, c.words * kValue);
                        rows.push_back({b, b + w});
                    }
                }
            }
            CHECK(j == c.first_job + c.njobs, "chunk has %zu jobs, its pairs %zu", c.njobs, j - c.first_job);
            std::sort(rows.begin(), rows.end());
            for (size_t r = 1; r < rows.size(); ++r) CHECK(rows[r - 1].second <= rows[r].first, "rows overlap at byte %zu", rows[r].first);
            next_pair += c.npairs;
            next_job += c.njobs;
        }
        CHECK(next_pair == np && next_job == P.jobs.size(), "chunks cover %zu pairs and %zu jobs", next_pair, next_job);
        CHECK(words_max == P.words_max, "words_max %zu, expected %zu", P.words_max, words_max);
        if (batch % 4 == 0) CHECK(P.chunks.size() == 1, "%zu chunks at a budget above the total", P.chunks.size());
        if (batch % 4 == 2 && total / 2 > biggest * 2) CHECK(P.chunks.size() >= 2, "one chunk at a budget of %zu for %zu bytes", budget, total);
    }
    std::printf("ok %d %d\n", batches, refused_batches);
    return 0;
}
