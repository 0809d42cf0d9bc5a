// affine_chain_plan.hpp -- the host-side plan of the chained gap-affine routes (affine_chain_kernel, affine_kernel.hpp, with 8-byte
// boundary values; affine4_chain_kernel, affine4_chain_kernel.hpp, with 16-byte ones).  Plain C++, no HIP: the unit tests compile it on
// its own.
//
// A pair with |b| > 1024 has S = ceil(|b| / 1024) strips.  Every strip is a job of its own; strip s < S - 1 owns one boundary row of
// |a| + 1 values of value_bytes bytes (8 unless the caller says otherwise), which strip s + 1 reads while strip s is still writing it.
// Sizes and offsets are counted in values; only the budget is in bytes.  Jobs are claimed by ticket in the order of the job
// list, so the list puts every pair's strips 0, 1, .. S - 1 next to each other in that order: a job's producer is the job before it.
// The pairs are cut, in the order given, into chunks whose boundary rows fit a byte budget; one chunk is one launch over one allocation.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pa {
namespace affine_chain {

constexpr uint32_t kStripRows = 1024;  // rows of one strip: 64 lanes x 16 rows (affine_kernel.hpp)

struct Shape {
    uint32_t n, m;  // |a|, |b| (|b| > kStripRows)
};

struct Job {
    uint32_t pair;   // index into the shapes given to plan()
    uint32_t strip;  // 0 .. strips - 1
};

// One launch: pairs [first_pair, first_pair + npairs), jobs [first_job, first_job + njobs) of Plan::jobs, `words` values of rows.
struct Chunk {
    size_t first_pair = 0, npairs = 0;
    size_t first_job = 0, njobs = 0;
    size_t words = 0;
};

struct Plan {
    std::vector<Job> jobs;        // ticket order, chunk after chunk
    std::vector<size_t> row_off;  // per pair: where in its chunk's allocation the row of strip 0 starts (in values); strip s at
                                  // row_off + s (n + 1)
    std::vector<Chunk> chunks;
    long long refused = -1;  // the first pair whose rows alone exceed the budget (then nothing else is valid), else -1
    size_t words_max = 0;    // the largest chunk's rows
};

inline size_t strips_of(uint32_t m) { return ((size_t)m + kStripRows - 1) / kStripRows; }
inline size_t row_words(uint32_t n) { return (size_t)n + 1; }
// Boundary rows of one pair, in values: every strip but the last keeps one.  (The count does not depend on the value's size.)
inline size_t pair_words(Shape p, size_t /*value_bytes*/ = 8) { return (strips_of(p.m) - 1) * row_words(p.n); }
inline size_t pair_bytes(Shape p, size_t value_bytes = 8) { return pair_words(p, value_bytes) * value_bytes; }

inline Plan plan(const std::vector<Shape>& pairs, size_t budget_bytes, size_t value_bytes = 8) {
    Plan P;
    const size_t budget_words = budget_bytes / value_bytes;
    for (size_t p = 0; p < pairs.size(); ++p)
        if (pair_words(pairs[p]) > budget_words) {
            P.refused = (long long)p;
            return P;
        }
    P.row_off.resize(pairs.size());
    for (size_t p = 0; p < pairs.size(); ++p) {
        const size_t w = pair_words(pairs[p]);
        if (P.chunks.empty() || P.chunks.back().words + w > budget_words) {
            Chunk c;
            c.first_pair = p;
            c.first_job = P.jobs.size();
            P.chunks.push_back(c);
        }
        Chunk& c = P.chunks.back();
        P.row_off[p] = c.words;
        c.words += w;
        c.npairs += 1;
        const size_t S = strips_of(pairs[p].m);
        for (size_t s = 0; s < S; ++s) P.jobs.push_back(Job{(uint32_t)p, (uint32_t)s});
        c.njobs += S;
        if (c.words > P.words_max) P.words_max = c.words;
    }
    return P;
}

}  // namespace affine_chain
}  // namespace pa
