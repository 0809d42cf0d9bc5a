// affine4_batch.hpp -- the host side that the two double-affine units share: the batch itself and the helpers of affine4_unit.hip
// (create, run, align, info) that affine4_tiled_unit.hip (align_tiled, tiled_info) needs too.  No kernel is defined or launched here.
#pragma once
#include "pa_hip_internal.hpp"
#include "affine4_common.hpp"

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

namespace pa {
namespace affine4 {

constexpr size_t kStripRows = 64 * kRows;  // rows of one strip

inline int seg_lg(size_t m) {  // log2 of the segment width: smallest g = 2^lg with g kRows >= m
    int lg = 0;
    while ((size_t(kRows) << lg) < m) ++lg;
    return lg;
}
inline size_t strips_of(uint32_t m) { return m <= kStripRows ? 1 : (m + kStripRows - 1) / kStripRows; }
inline size_t rows_of(uint32_t m) { return m <= kStripRows ? size_t(kRows) << seg_lg(m) : strips_of(m) * kStripRows; }  // H

// One launch's worth of waves over a subset of the pairs.
struct Plan {
    std::vector<Wave> waves;
    std::vector<Pair> pairs;
    size_t bnd_vals = 0, code_bytes = 0;  // bnd_vals: 16-byte boundary values
    double lanes = 0, slots = 0;
    size_t packed = 0, strip = 0;
    DeviceBuf d_waves, d_pairs, d_bnd;
};

}  // namespace affine4
}  // namespace pa

struct pa_affine4_batch {
    size_t np = 0;
    bool trace = false;
    pa::affine4::Costs C{};
    std::vector<uint32_t> n, m;
    std::vector<size_t> aoff, boff;  // offsets of a and b in d_seq
    std::vector<uint32_t> order;     // the planner's order: packed pairs by (g, |a|), then strip pairs by |a|
    pa::DeviceBuf d_seq, d_cost;
    pa::affine4::Plan fwd;
    double trace_chunks = 0;
    struct {
        double chunks = 0, rounds = 0, tile_jobs = 0, refill_cells = 0, chunk_bytes_max = 0;
    } tiled;  // the last align_tiled()
};

namespace pa {
namespace affine4 {

// The CIGAR text of a walk's ops (recorded from the end backwards): equal ops merge, the ops of every layer print as I / D.
inline std::string cigar_of(const uint8_t* op, int32_t nops) {
    std::string out;
    char num[16];
    for (int32_t x = nops - 1; x >= 0;) {
        int32_t y = x;
        while (y >= 0 && op[y] == op[x]) --y;
        const int32_t k = x - y;
        if (k > 1) {
            std::snprintf(num, sizeof num, "%d", k);
            out += num;
        }
        const uint8_t c = op[x];
        out += c == 'i' || c == 'j' ? 'I' : c == 'd' || c == 'e' ? 'D' : (char)c;
        x = y;
    }
    return out;
}

struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    bool make() {
        for (auto& x : e)
            if (!hip_ok(hipEventCreate(&x), "hipEventCreate")) return false;
        return true;
    }
    ~Events() {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// The costs of every pair, to the caller.
inline int costs_out(pa_affine4_batch& ab, int32_t* cost_out, hipStream_t s) {
    if (!cost_out || ab.np == 0) return 0;
    if (!hip_ok(hipMemcpyAsync(cost_out, ab.d_cost.ptr, ab.np * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    return 0;
}

}  // namespace affine4
}  // namespace pa
