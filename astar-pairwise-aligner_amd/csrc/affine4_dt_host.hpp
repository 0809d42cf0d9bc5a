// affine4_dt_host.hpp -- what the two units of the double-affine diagonal-transition route share on the host: the state a batch keeps
// for the route (affine4_dt_view.hpp declares it; affine4_dt_unit.hip releases it), the bound's limit, and the CIGAR text of a walk.
// affine4_dt_unit.hip has run_dt / align_dt and their _ends forms, affine4_dt_seg_unit.hip the segmented traceback.
#pragma once
#include "pa_hip_internal.hpp"
#include "affine4_dt_view.hpp"

#include <cstdint>
#include <cstdio>
#include <string>

namespace pa {
namespace affine4 {

struct DtState {
    DeviceBuf d_seq;  // the batch's sequences, with kSeqPad bytes after the last
    bool seq_ready = false;
    DeviceBuf d_cost, d_stat, d_jobs, d_fronts, d_wout;
    double found = 0, not_found = 0, chunks = 0, front_cells = 0, extend_chars = 0, bytes_max = 0;  // the last DT call
    DeviceBuf d_seg_jobs, d_seg_state, d_seg_stat;
    double seg_chunks = 0, seg_rounds = 0, seg_jobs = 0, seg_refill_cells = 0, seg_bytes_max = 0;  // the last align_dt_seg
};

constexpr int32_t kSMaxLimit = 1 << 30;

// The CIGAR text of a walk's ops (recorded from the end backwards): equal ops merge, the ops of every layer print as I / D
// (affine4_batch.hpp's cigar_of, restated: that header is the DP units').
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

}  // namespace affine4
}  // namespace pa
