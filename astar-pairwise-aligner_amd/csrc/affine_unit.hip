// affine_unit.hip -- batched gap-affine global alignment (pa_affine_batch_*, include/pa_affine_hip.h).
//
// NW::new(cm, false, false).align(a, b) of pa-base-algos (full-matrix AffineFront, nw/affine.rs) for many independent pairs, over the
// cost models AffineCost<0> and AffineCost<2> can express (pa-affine-types/src/cost_model.rs:112-190).  Every sequence is uploaded
// once.  run() launches affine_kernel<false> (costs only) over a plan made at creation: short pairs packed into segments, longer ones a
// wavefront each, most expensive waves first.  align() re-runs the pairs with affine_kernel<true> in chunks whose traceback codes (one
// byte per cell) fit a device-memory budget, and walks every pair's codes on the GPU (affine_walk_kernel).  align_tiled() gives the same
// CIGARs in bounded memory: a cost-only pass that keeps checkpoints (affine_ckpt_kernel), then rounds that re-fill the one tile of codes
// each unfinished pair's walk stands in (affine_tile_kernel) and walk it (affine_tile_walk_kernel).  set_chain(1) sends the pairs with
// |b| > 1024 through affine_chain_kernel in run() and in align_tiled()'s checkpoint pass: a wavefront per strip, the strips of a pair
// chained through their boundary rows (planned by affine_chain_plan.hpp).  set_free_ends() makes the ends of a free in all of these
// routes: the launches then pick the kernels' ENDS instantiations, which leave every pair's end in d_end; the walks start there, and
// pa_affine_batch_ends reports where they started and stopped.  last_row() is a cost-only pass of its own that also stores row |b|.
// The diagonal-transition route (run_dt, align_dt) is a unit of its own, affine_dt_unit.hip, which sees a batch through dt_view();
// local alignment (run_local, align_local) likewise, affine_local_unit.hip through local_view().
// The plan, the chunking and the drivers of align() and align_tiled() are affine_host.hpp's and the chained route's host side is
// affine_chain_host.hpp's, both shared with the four-layer batch, as is the host side of ends-free mode and last_row(); this unit gives
// them its records and launches (Host) and keeps what only two layers have: dt_view().
#include "engine.hpp"
#include "affine_kernel.hpp"
#include "affine_chain_host.hpp"
#include "affine_dt_view.hpp"
#include "affine_local_view.hpp"
#include "../../include/pa_affine_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace pa;
using namespace pa::affine;

namespace {

constexpr uint32_t kMaxCost = 1000;

using Plan = affine_host::Plan<Pair, Wave>;

}  // namespace

struct pa_affine_batch : affine_host::Batch<Pair, Wave> {
    Costs C{};
    // The chained route (set_chain): the packed pairs keep a plan of their own, the others are listed in planner order.
    affine_host::ChainState<Plan> chain;
    // Ends-free mode (set_free_ends): the switches are C.ends, the kernels leave every pair's end in d_end.
    DeviceBuf d_end;
    affine_host::EndsState ends;
    DtState* dt = nullptr;  // the diagonal-transition route's own state (affine_dt_unit.hip)
    LocalInfo local;        // the shape of the last align_local() (affine_local_unit.hip)
};

// What the local-alignment route (run_local, align_local: affine_local_unit.hip) reads of a batch.
LocalView pa::affine::local_view(pa_affine_batch* ab) { return LocalView{ab, ab->C, &ab->local}; }

// What the diagonal-transition route (run_dt, align_dt: affine_dt_unit.hip) reads of a batch.
DtView pa::affine::dt_view(pa_affine_batch* ab) {
    static_assert(kDtAbsent == kInf, "an absent edge");
    const Costs& C = ab->C;
    const size_t seq_bytes = ab->np ? ab->boff[ab->np - 1] + ab->m[ab->np - 1] : 0;  // (b of the last pair ends d_seq)
    return DtView{ab->np, ab->trace, DtCosts{C.sub, C.ins, C.del, C.io, C.ie, C.dopen, C.de, C.ends}, ab->n.data(), ab->m.data(),
                  ab->aoff.data(), ab->boff.data(), ab->d_seq.as<uint8_t>(), seq_bytes, &ab->dt};
}

namespace {

static_assert(kFreeStart == affine_host::kFreeStart && kFreeEnd == affine_host::kFreeEnd, "affine_host.hpp restates the switches");

// What affine_host.hpp's templates need of this batch type (the list is at the top of that header).
struct Host {
    using Batch = pa_affine_batch;
    using Pair = affine::Pair;
    using Wave = affine::Wave;
    using Walk = affine::Walk;
    using WalkOut = affine::WalkOut;
    using WalkState = affine::WalkState;
    using TileJob = affine::TileJob;
    using TileWave = affine::TileWave;
    using ChainJob = affine::ChainJob;
    // 8-byte boundary values (M | I << 32) and checkpoint rows (M | D << 32): a pair's checkpoints are whole 8-byte values as they are
    static constexpr affine_plan::Layout kLayout{kRows, 8, 8, 8};
    static_assert(kLayout.rows == kLocalLayout.rows && kLayout.bnd_bytes == kLocalLayout.bnd_bytes, "affine_local_view.hpp restates the layout");
    static constexpr const char* kName = "pa_affine_batch";
    static constexpr int32_t kMaxLayer = 2;
    static constexpr uint32_t kVisitSlack = 1;

    template <bool FILL>
    static bool launch(const Batch& ab, const Plan& P, hipStream_t s);
    static void walk_extra(const Batch& ab, const Pair& Q, Walk& w) {
        w.out = Q.out;
        w.free_start = ab.C.ends & kFreeStart;
    }
    static bool launch_walk(const Batch& ab, const Walk* d_walks, int nw, WalkOut* d_outs, hipStream_t s) {
        hipLaunchKernelGGL(affine_walk_kernel, dim3((nw + 63) / 64), dim3(64), 0, s, d_walks, nw, d_outs,
                           (ab.C.ends & kFreeEnd) ? ab.d_end.as<int32_t>() : nullptr);
        return hip_ok(hipGetLastError(), "affine_walk_kernel launch");
    }
    static int64_t walk_start(const WalkOut& o) { return o.start; }
    static void begin_tiled(Batch& ab) { affine_host::chain_begin(ab); }
    static int ckpt_pass(Batch& ab, affine_host::TiledChunk<Host>& ch, uint32_t C, hipStream_t s, float* ms) {
        return affine_host::ckpt_pass<Host>(ab, ch, C, s, ms);
    }
    static uint32_t ends_flags(const Batch& ab) { return ab.C.ends; }
    static void set_ends_flags(Batch& ab, uint32_t f) { ab.C.ends = f; }
    static bool launch_rows(const Batch& ab, const Plan& P, int32_t* d_rows, const uint64_t* d_off, hipStream_t s);
    // what affine_chain_host.hpp launches
    static bool launch_ckpt(const Batch& ab, const Wave* d_waves, size_t nwaves, const Pair* d_pairs, hipStream_t s);
    template <bool CKPT>
    static bool launch_chain(const Batch& ab, const ChainJob* d_jobs, int njobs, const Pair* d_pairs, uint32_t tile_cols, uint32_t* ticket_err, hipStream_t s);
    static bool launch_chain_run(const Batch& ab, const ChainJob* d_jobs, int njobs, const Pair* d_pairs, uint32_t* ticket_err, hipStream_t s) {
        return launch_chain<false>(ab, d_jobs, njobs, d_pairs, 0, ticket_err, s);
    }
    static bool launch_chain_ckpt(const Batch& ab, const ChainJob* d_jobs, int njobs, const Pair* d_pairs, uint32_t tile_cols, uint32_t* ticket_err,
                                  hipStream_t s) {
        return launch_chain<true>(ab, d_jobs, njobs, d_pairs, tile_cols, ticket_err, s);
    }
    static bool launch_tile_fill(const Batch& ab, const TileWave* d_waves, int nw, const TileJob* d_jobs, hipStream_t s);
    static bool launch_tile_walk(const Batch& ab, const TileJob* d_jobs, int nj, hipStream_t s) {
        hipLaunchKernelGGL(affine_tile_walk_kernel, dim3((nj + 63) / 64), dim3(64), 0, s, d_jobs, nj, (ab.C.ends & kFreeStart) ? 1 : 0);
        return hip_ok(hipGetLastError(), "affine_tile_walk_kernel launch");
    }
    static bool walk_done(const Batch& ab, const WalkState& S) { return S.j == 0 && S.layer == 0 && (S.i == 0 || (ab.C.ends & kFreeStart)); }
    // The CIGAR text of a walk's ops (recorded from the end backwards).
    static std::string cigar_of(const uint8_t* op, int32_t nops) {
        engine::Cigar cig;
        for (int32_t x = 0; x < nops; ++x) {
            const engine::CigarOp c = op[x] == '=' ? engine::CigarOp::Match
                                      : op[x] == 'X' ? engine::CigarOp::Sub
                                      : op[x] == 'D' ? engine::CigarOp::Del
                                                     : engine::CigarOp::Ins;
            cig.push_elem(engine::CigarElem{c, 1});
        }
        cig.reverse();
        return cig.to_string();
    }
    static int finish(Batch& ab, int32_t* cost_out, hipStream_t s, const std::vector<int64_t>* starts) {
        return affine_host::costs_out<Host>(ab, cost_out, s, starts);
    }
};

// affine_kernel over nwaves device waves; a whole plan's, or (the checkpoint pass with chaining on) the one-strip waves of a plan.
// Global mode runs the instantiations without the ends-free state; a free end, or `rows` (last_row(): where the last rows go), the ones with.
Ends ends_of(const pa_affine_batch& ab, const Ends* rows = nullptr) {
    Ends E{ab.d_end.as<int32_t>(), nullptr, nullptr};
    return rows ? *rows : E;
}
template <bool FILL, bool CKPT = false>
bool launch(const pa_affine_batch& ab, const Wave* d_waves, size_t nwaves, const Pair* d_pairs, hipStream_t s, const Ends* rows = nullptr) {
    if (nwaves == 0) return true;
    const int grid = (int)((nwaves + kBlockWaves - 1) / kBlockWaves);
    if (ab.C.ends || rows)
        hipLaunchKernelGGL((affine_kernel<FILL, CKPT, true>), dim3(grid), dim3(64 * kBlockWaves), 0, s, d_waves, (int)nwaves, d_pairs, ab.C,
                           ab.d_cost.as<int32_t>(), ends_of(ab, rows));
    else
        hipLaunchKernelGGL((affine_kernel<FILL, CKPT, false>), dim3(grid), dim3(64 * kBlockWaves), 0, s, d_waves, (int)nwaves, d_pairs, ab.C,
                           ab.d_cost.as<int32_t>(), Ends{});
    return hip_ok(hipGetLastError(), FILL ? "affine_kernel<FILL> launch" : CKPT ? "affine_kernel<CKPT> launch" : "affine_kernel launch");
}
template <bool FILL>
bool launch(const pa_affine_batch& ab, const Plan& P, hipStream_t s) {
    return launch<FILL>(ab, P.d_waves.as<Wave>(), P.waves.size(), P.d_pairs.as<Pair>(), s);
}
template <bool FILL>
bool Host::launch(const Batch& ab, const Plan& P, hipStream_t s) {
    return ::launch<FILL>(ab, P, s);
}

bool Host::launch_ckpt(const Batch& ab, const Wave* d_waves, size_t nwaves, const Pair* d_pairs, hipStream_t s) {
    return ::launch<false, true>(ab, d_waves, nwaves, d_pairs, s);
}
// affine_chain_kernel over one chunk's jobs (the chained route's host side is affine_chain_host.hpp's).
template <bool CKPT>
bool Host::launch_chain(const Batch& ab, const ChainJob* d_jobs, int njobs, const Pair* d_pairs, uint32_t tile_cols, uint32_t* ticket_err, hipStream_t s) {
    const int grid = (njobs + kBlockWaves - 1) / kBlockWaves;
    if (ab.C.ends)
        hipLaunchKernelGGL((affine_chain_kernel<CKPT, true>), dim3(grid), dim3(64 * kBlockWaves), 0, s, d_jobs, njobs, d_pairs, ab.C, tile_cols, ticket_err,
                           ab.d_cost.as<int32_t>(), ends_of(ab));
    else
        hipLaunchKernelGGL((affine_chain_kernel<CKPT, false>), dim3(grid), dim3(64 * kBlockWaves), 0, s, d_jobs, njobs, d_pairs, ab.C, tile_cols, ticket_err,
                           ab.d_cost.as<int32_t>(), Ends{});
    return hip_ok(hipGetLastError(), CKPT ? "affine_chain_kernel<CKPT> launch" : "affine_chain_kernel launch");
}

using affine_host::Events;

// last_row(): the cost-only ENDS kernel over a plan, the last rows to d_rows.
bool Host::launch_rows(const Batch& ab, const Plan& P, int32_t* d_rows, const uint64_t* d_off, hipStream_t s) {
    const Ends E{ab.d_end.as<int32_t>(), d_rows, d_off};
    return ::launch<false>(ab, P.d_waves.as<Wave>(), P.waves.size(), P.d_pairs.as<Pair>(), s, &E);
}

}  // namespace

extern "C" pa_affine_batch* pa_affine_batch_create(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b, const size_t* b_len,
                                                   size_t npairs, const pa_affine_cost* cm, int trace) {
    if (!cm) {
        set_error("pa_affine_batch_create: NULL cost model");
        return nullptr;
    }
    if (npairs && (!a || !a_len || !b || !b_len)) {
        set_error("pa_affine_batch_create: NULL array");
        return nullptr;
    }
    // the cost model (AffineCost::new, cost_model.rs:229-242): every present cost >= 1, here also <= 1000; 0 = absent
    const int32_t f[7] = {cm->sub, cm->ins, cm->del, cm->ins_open, cm->ins_extend, cm->del_open, cm->del_extend};
    static const char* names[7] = {"sub", "ins", "del", "ins_open", "ins_extend", "del_open", "del_extend"};
    for (int k = 0; k < 7; ++k)
        if (f[k] < 0 || f[k] > (int32_t)kMaxCost) {
            set_error("pa_affine_batch_create: cost %s = %d outside [1, %u] (0 = absent)", names[k], f[k], kMaxCost);
            return nullptr;
        }
    if ((cm->ins_open == 0) != (cm->ins_extend == 0) || (cm->del_open == 0) != (cm->del_extend == 0)) {
        set_error("pa_affine_batch_create: an affine layer needs both open and extend");
        return nullptr;
    }
    const bool ins_layer = cm->ins_open != 0, del_layer = cm->del_open != 0;
    if (!cm->ins && !ins_layer) {
        set_error("pa_affine_batch_create: the cost model has no insertion edge");
        return nullptr;
    }
    if (!cm->del && !del_layer) {
        set_error("pa_affine_batch_create: the cost model has no deletion edge");
        return nullptr;
    }
    const uint64_t max_edge = std::max({(uint64_t)cm->sub, (uint64_t)cm->ins, (uint64_t)cm->del, (uint64_t)cm->ins_open + (uint64_t)cm->ins_extend,
                                        (uint64_t)cm->del_open + (uint64_t)cm->del_extend});
    auto cost = [](int32_t c) { return c ? (uint32_t)c : kInf; };
    const Costs C{cost(cm->sub), cost(cm->ins), cost(cm->del), cost(cm->ins_open), cost(cm->ins_extend), cost(cm->del_open), cost(cm->del_extend), 0};
    return affine_host::create<Host>(a, a_len, b, b_len, npairs, trace, max_edge, C);
}

extern "C" int pa_affine_batch_run(pa_affine_batch* ab, int32_t* cost_out, float* kernel_ms) {
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_run: NULL batch");
    if (kernel_ms) *kernel_ms = 0;
    hipStream_t s = 0;
    if (ab->np == 0) return Host::finish(*ab, cost_out, s, nullptr);  // (nothing to copy: the call counts for pa_affine_batch_ends)
    Events ev;
    if (!ev.make()) return PA_E_HIP;
    affine_host::chain_begin(*ab);
    if (ab->chain.on && !ab->chain.ids.empty()) {
        if (const int rc = affine_host::run_chained<Host>(*ab, ev, s)) return rc;
    } else if (!hip_ok(hipEventRecord(ev.e[0], s), "event") || !launch<false>(*ab, ab->fwd, s) || !hip_ok(hipEventRecord(ev.e[1], s), "event"))
        return PA_E_HIP;
    if (const int rc = Host::finish(*ab, cost_out, s, nullptr)) return rc;
    if (kernel_ms && !hip_ok(hipEventElapsedTime(kernel_ms, ev.e[0], ev.e[1]), "hipEventElapsedTime")) return PA_E_HIP;
    return 0;
}

extern "C" int pa_affine_batch_align(pa_affine_batch* ab, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    return affine_host::align<Host>(ab, cost_out, cigar_out, forward_ms, trace_ms);
}

namespace {

// The fill of a round's tiles.  FS: row 0 is zero in every column, as the checkpoint pass had it.
bool Host::launch_tile_fill(const Batch& ab, const TileWave* d_waves, int nw, const TileJob* d_jobs, hipStream_t s) {
    hipLaunchKernelGGL((ab.C.ends & kFreeStart) ? affine_tile_kernel<true> : affine_tile_kernel<false>, dim3((nw + kBlockWaves - 1) / kBlockWaves),
                       dim3(64 * kBlockWaves), 0, s, d_waves, nw, d_jobs, ab.C);
    return hip_ok(hipGetLastError(), "affine_tile_kernel launch");
}

}  // namespace

extern "C" int pa_affine_batch_align_tiled(pa_affine_batch* ab, uint32_t tile_cols, int32_t* cost_out, char** cigar_out, float* forward_ms,
                                           float* refill_ms, float* walk_ms) {
    return affine_host::align_tiled<Host>(ab, tile_cols, cost_out, cigar_out, forward_ms, refill_ms, walk_ms);
}

extern "C" void pa_affine_batch_tiled_info(const pa_affine_batch* ab, double* chunks, double* rounds, double* tile_jobs, double* refill_cells,
                                           double* chunk_bytes_max) {
    affine_host::tiled_info(ab, chunks, rounds, tile_jobs, refill_cells, chunk_bytes_max);
}

extern "C" int pa_affine_batch_set_chain(pa_affine_batch* ab, int on) {
    return affine_host::set_chain<Host>(ab, on);
}

extern "C" int pa_affine_batch_set_free_ends(pa_affine_batch* ab, int free_start, int free_end) {
    return affine_host::set_free_ends<Host>(ab, free_start, free_end);
}

extern "C" int pa_affine_batch_ends(const pa_affine_batch* ab, int64_t* start_out, int64_t* end_out) {
    return affine_host::batch_ends<Host>(ab, start_out, end_out);
}

extern "C" int pa_affine_batch_last_row(pa_affine_batch* ab, int32_t* out, const uint64_t* offsets) {
    return affine_host::last_row<Host>(ab, out, offsets);
}

extern "C" void pa_affine_batch_chain_info(const pa_affine_batch* ab, double* on, double* chain_pairs, double* chain_jobs, double* chunks,
                                           double* bnd_bytes_max) {
    affine_host::chain_info(ab, on, chain_pairs, chain_jobs, chunks, bnd_bytes_max);
}

extern "C" void pa_affine_batch_info(const pa_affine_batch* ab, double* waves, double* packed_pairs, double* strip_pairs, double* lane_use,
                                     double* trace_chunks) {
    affine_host::batch_info(ab, waves, packed_pairs, strip_pairs, lane_use, trace_chunks);
}

extern "C" void pa_affine_batch_destroy(pa_affine_batch* ab) {
    if (!ab) return;
    (void)hipDeviceSynchronize();
    dt_release(ab->dt);
    delete ab;
}
