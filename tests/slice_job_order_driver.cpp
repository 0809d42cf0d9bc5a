// Stand-alone check of csrc/slice_job_order.hpp (tests/test_slice_job_order.py builds it with the address and undefined-behaviour
// sanitizers and runs it): seeded random plans against the properties the bit-sliced kernel's ticket order relies on.  Exit status 0 and
// "ok <plans>" when every property held, else the first violation on stderr and status 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "slice_job_order.hpp"

using namespace pa::slice;

#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            std::fprintf(stderr, "plan %d: ", plan);     \
            std::fprintf(stderr, __VA_ARGS__);           \
            std::fprintf(stderr, " (%s)\n", #cond);      \
            return 1;                                    \
        }                                                \
    } while (0)

static bool same(const std::vector<SliceJob>& x, const std::vector<SliceJob>& y) {
    if (x.size() != y.size()) return false;
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i].group != y[i].group || x[i].strip != y[i].strip) return false;
    return true;
}

// written out here, not taken from the header
static std::vector<SliceJob> group_major(const std::vector<int>& nstrips) {
    std::vector<SliceJob> j;
    for (size_t g = 0; g < nstrips.size(); ++g)
        for (int s = 0; s < nstrips[g]; ++s) j.push_back(SliceJob{(uint32_t)g, (uint32_t)s});
    return j;
}
static std::vector<SliceJob> strip_major(const std::vector<int>& nstrips) {
    std::vector<SliceJob> j;
    const int longest = *std::max_element(nstrips.begin(), nstrips.end());
    for (int s = 0; s < longest; ++s)
        for (size_t g = 0; g < nstrips.size(); ++g)
            if (s < nstrips[g]) j.push_back(SliceJob{(uint32_t)g, (uint32_t)s});
    return j;
}

int main() {
    std::mt19937_64 rng(20241019);
    const int plans = 400;
    const int chains[] = {0, 1, 2, 3, 8, -1};
    for (int plan = 0; plan < plans; ++plan) {
        const size_t groups = 1 + rng() % 300;
        std::vector<int> nstrips(groups);
        for (int& s : nstrips) s = 1 + (int)(rng() % 40);
        if (plan % 5 == 0) std::sort(nstrips.begin(), nstrips.end(), [](int x, int y) { return x > y; });  // heaviest first, as the plan has them
        const size_t slots = 1 + rng() % 4096;
        const int longest = *std::max_element(nstrips.begin(), nstrips.end());
        size_t total = 0;
        std::vector<size_t> first(groups + 1, 0);  // (group, strip) -> index
        for (size_t g = 0; g < groups; ++g) {
            first[g] = total;
            total += (size_t)nstrips[g];
        }
        // the automatic chain length: clamp(ceil(slots / groups), 1, longest)
        const int C_auto = auto_chain(nstrips, slots);
        {
            size_t c = slots / groups + (slots % groups != 0);
            if (c < 1) c = 1;
            if (c > (size_t)longest) c = (size_t)longest;
            CHECK(C_auto == (int)c, "automatic chain %d, expected %zu", C_auto, c);
        }
        for (const int chain : chains) {
            const std::vector<SliceJob> jobs = job_order(nstrips, slots, chain);
            int C = chain < 0 ? C_auto : chain;
            if (C == 0 || C > longest) C = longest;
            // a permutation of all (group, strip)
            CHECK(jobs.size() == total, "chain %d: %zu jobs for %zu strips", chain, jobs.size(), total);
            std::vector<long long> ticket(total, -1);
            for (size_t t = 0; t < jobs.size(); ++t) {
                CHECK(jobs[t].group < groups, "chain %d ticket %zu: group %u", chain, t, jobs[t].group);
                CHECK((int)jobs[t].strip < nstrips[jobs[t].group], "chain %d ticket %zu: strip %u of %d", chain, t, jobs[t].strip, nstrips[jobs[t].group]);
                long long& at = ticket[first[jobs[t].group] + jobs[t].strip];
                CHECK(at < 0, "chain %d ticket %zu: group %u strip %u twice", chain, t, jobs[t].group, jobs[t].strip);
                at = (long long)t;
            }
            // every strip's producer has a lower ticket
            for (size_t g = 0; g < groups; ++g)
                for (int s = 1; s < nstrips[g]; ++s)
                    CHECK(ticket[first[g] + s - 1] < ticket[first[g] + s], "chain %d: group %zu strip %d before its producer", chain, g, s);
            // bands in ascending order; within a band the groups in plan order, and a group's strips contiguous and ascending
            for (size_t t = 1; t < jobs.size(); ++t) {
                const SliceJob p = jobs[t - 1], j = jobs[t];
                const int bp = (int)p.strip / C, bj = (int)j.strip / C;
                CHECK(bp <= bj, "chain %d ticket %zu: band %d after band %d", chain, t, bj, bp);
                if (bp == bj) {
                    CHECK(p.group <= j.group, "chain %d ticket %zu: group %u after group %u in band %d", chain, t, j.group, p.group, bj);
                    if (p.group == j.group) CHECK(j.strip == p.strip + 1, "chain %d ticket %zu: strip %u after strip %u", chain, t, j.strip, p.strip);
                }
                if (p.group != j.group || bp != bj) {  // a group's run in a band starts at the band's first strip and the one before ended at its last
                    CHECK((int)j.strip == bj * C, "chain %d ticket %zu: the run starts at strip %u", chain, t, j.strip);
                    CHECK((int)p.strip == std::min(bp * C + C, nstrips[p.group]) - 1, "chain %d ticket %zu: the run ended at strip %u", chain, t, p.strip);
                }
            }
            if (chain == 0) CHECK(same(jobs, group_major(nstrips)), "chain 0 is not group-major");
            if (chain == 1) CHECK(same(jobs, strip_major(nstrips)), "chain 1 is not strip-major");
        }
        // any C >= the longest group is one band
        CHECK(same(job_order(nstrips, slots, longest), group_major(nstrips)), "chain = longest is not group-major");
        CHECK(same(job_order(nstrips, slots, longest + 1 + (int)(rng() % 100)), group_major(nstrips)), "chain > longest is not group-major");
    }
    const int plan = -1;
    {  // the bench batch: 256 groups of 32 strips on 2048 wave slots = four bands of 2048 jobs, chains of 8
        const std::vector<int> nstrips(256, 32);
        CHECK(auto_chain(nstrips, 2048) == 8, "bench batch: automatic chain %d", auto_chain(nstrips, 2048));
        const std::vector<SliceJob> jobs = job_order(nstrips, 2048, -1);
        CHECK(jobs.size() == 8192, "bench batch: %zu jobs", jobs.size());
        for (size_t t = 0; t < jobs.size(); ++t) {
            CHECK(jobs[t].strip / 8 == t / 2048, "bench batch: ticket %zu is strip %u", t, jobs[t].strip);
            CHECK(jobs[t].group == (t % 2048) / 8 && jobs[t].strip % 8 == t % 8, "bench batch: ticket %zu is group %u strip %u", t, jobs[t].group, jobs[t].strip);
        }
    }
    {  // 65 536 x 10 kbp: 2048 groups of 4 strips: nothing runs beside its producer's band
        const std::vector<int> nstrips(2048, 4);
        CHECK(auto_chain(nstrips, 2048) == 1, "2048 groups: automatic chain %d", auto_chain(nstrips, 2048));
        CHECK(same(job_order(nstrips, 2048, -1), strip_major(nstrips)), "2048 groups: not strip-major");
    }
    CHECK(job_order(std::vector<int>(), 2048, -1).empty() && auto_chain(std::vector<int>(), 2048) == 0, "no groups");
    std::printf("ok %d\n", plans);
    return 0;
}
