// slice_job_order.hpp -- the TICKET ORDER of the bit-sliced kernel's (group, strip) jobs (slice_kernel.hpp).  Plain C++, no HIP: the unit
// tests compile it on its own.
//
// The wavefronts of a launch claim jobs by an atomic ticket, in the order of the job list.  Strips that run at the same time, one behind
// the other, form a CHAIN: each polls the boundary row of the strip above, the chain runs at the pace of its slowest member and the
// others sleep the difference.  A group's boundary rows are stored in full, so a strip can just as well read a row that was finished
// long ago: the chain need not be the whole group.  The list is therefore cut into BANDS of C strips:
//     band b = 0, 1, ..;  within a band the groups in plan order (heaviest first);  within a group its strips [b C, min((b + 1) C, nstrips))
//     ascending.
// With `slots` wavefronts in flight and G groups, C = ceil(slots / G) fills the chip with one band: chains of C strips, whose heads find
// their input complete (or nearly: written by the tail of the band before).  C = 0 is ONE band -- group after group, all strips of each.
// C = 1 is strip-major: all groups' strip 0, then all groups' strip 1, ..; the strips of a group then follow each other as slots fall free.
//
// THE INVARIANT: strip s - 1 of a group (the producer of strip s) always holds a LOWER ticket than strip s.  Tickets are claimed in order
// by wavefronts that are already running, so a consumer's producer has always started, and every poll of a boundary row is bounded.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pa {
namespace slice {

struct SliceJob {
    uint32_t group, strip;
};

// The automatic chain length: one band fills the wave slots.  clamp(ceil(slots / groups), 1, longest group); 0 for no groups.  Whatever
// the bands, at least this many strips of a group run at the same time once the launch is under way.
inline int auto_chain(size_t groups, int longest, size_t slots) {
    if (groups == 0) return 0;
    const size_t c = (slots + groups - 1) / groups;
    return (int)std::min(std::max<size_t>(c, 1), (size_t)std::max(longest, 1));
}
inline int auto_chain(const std::vector<int>& nstrips, size_t slots) {
    return nstrips.empty() ? 0 : auto_chain(nstrips.size(), *std::max_element(nstrips.begin(), nstrips.end()), slots);
}

// nstrips[g]: strips of group g, in plan order.  chain: C > 0, 0 = one band, < 0 = auto_chain(nstrips, slots).
inline std::vector<SliceJob> job_order(const std::vector<int>& nstrips, size_t slots, int chain) {
    std::vector<SliceJob> jobs;
    if (nstrips.empty()) return jobs;
    const int longest = *std::max_element(nstrips.begin(), nstrips.end());
    int C = chain < 0 ? auto_chain(nstrips, slots) : chain;
    if (C == 0 || C > longest) C = std::max(longest, 1);
    size_t total = 0;
    for (const int s : nstrips) total += (size_t)std::max(s, 0);
    jobs.reserve(total);
    for (int lo = 0; lo < longest; lo += C)
        for (size_t g = 0; g < nstrips.size(); ++g)
            for (int s = lo; s < std::min(lo + C, nstrips[g]); ++s) jobs.push_back(SliceJob{(uint32_t)g, (uint32_t)s});
    return jobs;
}

}  // namespace slice
}  // namespace pa
