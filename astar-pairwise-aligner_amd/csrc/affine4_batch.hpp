// affine4_batch.hpp -- what the two double-affine units share: the batch, and the part of affine_host.hpp's traits that both
// affine4_unit.hip (create, run, align, info) and affine4_tiled_unit.hip (align_tiled, tiled_info) give.  Each unit adds the records and
// launches of its own kernels; no kernel is launched here.  The chained route (set_chain) is split the same way: its state is the
// batch's, its host side affine_chain_host.hpp's, and of affine4_chain_kernel<CKPT> (a template: each unit instantiates what it
// launches) affine4_unit.hip runs the cost-only form in run() and affine4_tiled_unit.hip the checkpointing one in align_tiled().
// affine4_local_unit.hip (run_local, align_local) reads the batch from here too and keeps one host-only slot in it, LocalInfo.
#pragma once
#include "affine4_common.hpp"
#include "affine4_chain_kernel.hpp"
#include "affine_chain_host.hpp"

#include <cstdio>
#include <string>
#include <vector>

namespace pa {
namespace affine4 {
struct DtState;  // affine4_dt_view.hpp
struct LocalInfo {
    double chunks = 0, bytes_max = 0;  // of the last align_local(): chunks, device bytes of traceback codes of the largest one
};
}
}  // namespace pa

struct pa_affine4_batch : pa::affine_host::Batch<pa::affine4::Pair, pa::affine4::Wave> {
    pa::affine4::Costs C{};
    pa::affine_host::ChainState<pa::affine_host::Plan<pa::affine4::Pair, pa::affine4::Wave>> chain;  // set_chain
    // Ends-free mode (set_free_ends, include/pa_affine4_ends_hip.h): the switches (kFreeStart | kFreeEnd; they reach the ENDS
    // instantiations in their Ends record, Costs stays as it is), and every pair's end as those kernels leave it.
    uint32_t free_ends = 0;
    pa::DeviceBuf d_end;
    pa::affine_host::EndsState ends;
    pa::affine4::DtState* dt = nullptr;  // the diagonal-transition route's own state (affine4_dt_unit.hip)
    pa::affine4::LocalInfo local;        // the shape of the last align_local() (affine4_local_unit.hip); host only
};

namespace pa {
namespace affine4 {

struct HostBase {
    using Batch = pa_affine4_batch;
    using Pair = affine4::Pair;
    using Wave = affine4::Wave;
    using ChainJob = affine4::ChainJob;
    // 16-byte boundary values {M, I1, I2, 0}, 12-byte checkpoint rows {M, D1, D2}; a pair's checkpoints are loaded as 16-byte values
    static constexpr affine_plan::Layout kLayout{kRows, 16, 12, 16};
    static constexpr const char* kName = "pa_affine4_batch";
    static constexpr int32_t kMaxLayer = 4;
    static constexpr uint32_t kVisitSlack = 0;

    // The CIGAR text of a walk's ops (recorded from the end backwards): equal ops merge, the ops of every layer print as I / D.
    static std::string cigar_of(const uint8_t* op, int32_t nops) {
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
    // Ends-free mode (the host side is affine_host.hpp's): the switches, the record the ENDS instantiations take, and the end of every
    // call, which keeps what pa_affine4_batch_ends reports.
    static uint32_t ends_flags(const Batch& ab) { return ab.free_ends; }
    static void set_ends_flags(Batch& ab, uint32_t f) { ab.free_ends = f; }
    static Ends ends_of(const Batch& ab) { return Ends{ab.d_end.as<int32_t>(), nullptr, nullptr, ab.free_ends}; }
    static int finish(Batch& ab, int32_t* cost_out, hipStream_t s, const std::vector<int64_t>* starts = nullptr) {
        return affine_host::costs_out<HostBase>(ab, cost_out, s, starts);
    }
};
static_assert(kFreeStart == affine_host::kFreeStart && kFreeEnd == affine_host::kFreeEnd, "affine_host.hpp restates the switches");

}  // namespace affine4
}  // namespace pa
