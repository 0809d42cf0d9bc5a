// Stand-alone driver of csrc/band_search.hpp (tests/test_band_search.py builds it with the address and undefined-behaviour sanitizers
// and runs it as a child process).  stdin: one scripted search per line,
//   <doubling 1|2> <start 0|1|2> <factor> <delta> <h0> <gap> <block width> <count> <outcome> x count
// where an outcome is -1 for None and the distance for Some(distance).  stdout, one line per search:
//   <bounds tried> <bound> x that <found 0|1> <cost, -1 if not found> <s afterwards> <sanity count>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <vector>

#include "band_search.hpp"

int main() {
    int doubling, start, count;
    float factor;
    int32_t delta, h0, gap, block_width;
    while (std::cin >> doubling >> start >> factor >> delta >> h0 >> gap >> block_width >> count) {
        std::vector<int32_t> outcomes((size_t)count);
        for (int32_t& o : outcomes) std::cin >> o;
        if (!std::cin) return 2;
        const pa::band::Schedule sc{(pa::band::DoublingKind)doubling, (pa::band::DoublingStart)start, factor, delta};
        pa::band::Search bs;
        bs.begin(sc, h0, gap, block_width);
        std::vector<int32_t> bounds;
        bool found = false;
        int32_t cost = -1;
        for (const int32_t o : outcomes) {
            bounds.push_back(bs.s);
            if (bs.record(sc, o >= 0, o, pa::band::HostUniform{})) {
                found = true;
                cost = o;
                break;
            }
        }
        std::printf("%zu", bounds.size());
        for (const int32_t b : bounds) std::printf(" %d", b);
        std::printf(" %d %d %d %u\n", found ? 1 : 0, cost, bs.s, bs.sanity);
    }
    return std::cin.eof() ? 0 : 2;
}
