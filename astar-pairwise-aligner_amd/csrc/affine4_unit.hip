// affine4_unit.hip -- batched double-affine global alignment (pa_affine4_batch_*, include/pa_affine4_hip.h).
//
// NW::new(cm, false, false).align(a, b) of pa-base-algos for many independent pairs under an AffineCost<4> with layers [insert, delete,
// insert, delete].  The shape of affine_unit.hip's global-mode routes: every sequence is uploaded once; run() launches
// affine4_kernel<false> (costs only) over a plan made at creation, short pairs packed into segments, longer ones a wavefront each, most
// expensive waves first; align() re-runs the pairs with affine4_kernel<true> in chunks whose traceback codes (one byte per cell) fit a
// device-memory budget, and walks every pair's codes on the GPU (affine4_walk_kernel).  align_tiled() is affine4_tiled_unit.hip; the
// batch is in affine4_batch.hpp, and the plan, the tail of create and the driver of align() are affine_host.hpp's, shared with the
// two-layer batch.  set_chain(1) (include/pa_affine4_chain_hip.h) sends the pairs with |b| > 1024 through affine4_chain_kernel<false>
// in run(), a wavefront per strip, the strips of a pair chained through their boundary rows; the host side of that route is
// affine_chain_host.hpp's, shared likewise.  set_free_ends() (include/pa_affine4_ends_hip.h) makes the ends of a free in all of these
// routes: the launches then pick the kernels' ENDS instantiations, which leave every pair's end in d_end; the walks start there, and
// pa_affine4_batch_ends reports where they started and stopped.  last_row() is a cost-only pass of its own that also stores row |b|.
// The host side of all three is affine_host.hpp's, shared with the two-layer batch.  The diagonal-transition route (run_dt, align_dt and
// their ends-free forms, include/pa_affine4_dt_hip.h) is a unit of its own, affine4_dt_unit.hip, which sees a batch through dt_view().
// Not supported: other layer lists.
#include "affine4_kernel.hpp"
#include "affine4_batch.hpp"
#include "affine4_dt_view.hpp"
#include "../../include/pa_affine4_chain_hip.h"
#include "../../include/pa_affine4_ends_hip.h"

#include <algorithm>

using namespace pa;
using namespace pa::affine4;

// What the diagonal-transition route (affine4_dt_unit.hip) reads of a batch: open_t = oe[t] - e[t].
DtView pa::affine4::dt_view(pa_affine4_batch* ab) {
    static_assert(dt::kAbsent == kInf, "an absent edge");
    const Costs& C = ab->C;
    dt::Costs D{C.sub, C.ins, C.del, {}, {}};
    for (int t = 0; t < 4; ++t) {
        D.open[t] = C.oe[t] - C.e[t];
        D.ext[t] = C.e[t];
    }
    const size_t seq_bytes = ab->np ? ab->boff[ab->np - 1] + ab->m[ab->np - 1] : 0;  // (b of the last pair ends d_seq)
    return DtView{ab->np, ab->trace, D, ab->free_ends, ab->n.data(), ab->m.data(), ab->aoff.data(), ab->boff.data(), ab->d_seq.as<uint8_t>(),
                  seq_bytes, &ab->dt};
}

namespace {

constexpr int32_t kMaxCost = 1000;

// affine_host.hpp's traits for the routes of this unit: run() and align().
struct Host : HostBase {
    using Walk = affine4::Walk;
    using WalkOut = affine4::WalkOut;

    template <bool FILL>
    static bool launch(const Batch& ab, const affine_host::Plan<Pair, Wave>& P, hipStream_t s) {
        if (P.waves.empty()) return true;
        return launch_ends<FILL>(ab, P, s, nullptr);
    }
    // Global mode runs the instantiation without the ends-free state; a free end, or `rows` (last_row(): where the last rows go), the one with.
    template <bool FILL>
    static bool launch_ends(const Batch& ab, const affine_host::Plan<Pair, Wave>& P, hipStream_t s, const Ends* rows) {
        const int grid = (int)((P.waves.size() + kBlockWaves - 1) / kBlockWaves);
        if (ab.free_ends || rows)
            hipLaunchKernelGGL((affine4_kernel<FILL, true>), dim3(grid), dim3(64 * kBlockWaves), 0, s, P.d_waves.as<Wave>(), (int)P.waves.size(),
                               P.d_pairs.as<Pair>(), ab.C, ab.d_cost.as<int32_t>(), rows ? *rows : ends_of(ab));
        else
            hipLaunchKernelGGL((affine4_kernel<FILL, false>), dim3(grid), dim3(64 * kBlockWaves), 0, s, P.d_waves.as<Wave>(), (int)P.waves.size(),
                               P.d_pairs.as<Pair>(), ab.C, ab.d_cost.as<int32_t>(), Ends{});
        return hip_ok(hipGetLastError(), FILL ? "affine4_kernel<FILL> launch" : "affine4_kernel launch");
    }
    static bool launch_rows(const Batch& ab, const affine_host::Plan<Pair, Wave>& P, int32_t* d_rows, const uint64_t* d_off, hipStream_t s) {
        if (P.waves.empty()) return true;
        const Ends E{ab.d_end.as<int32_t>(), d_rows, d_off, ab.free_ends};
        return launch_ends<false>(ab, P, s, &E);
    }
    static void walk_extra(const Batch&, const Pair& Q, Walk& w) {
        w.out = Q.out;
        w.pad_ = 0;
    }
    static bool launch_walk(const Batch& ab, const Walk* d_walks, int nw, WalkOut* d_outs, hipStream_t s) {
        hipLaunchKernelGGL(affine4_walk_kernel, dim3((nw + 63) / 64), dim3(64), 0, s, d_walks, nw, d_outs,
                           (ab.free_ends & kFreeEnd) ? ab.d_end.as<int32_t>() : nullptr, (ab.free_ends & kFreeStart) ? 1 : 0);
        return hip_ok(hipGetLastError(), "affine4_walk_kernel launch");
    }
    static int64_t walk_start(const WalkOut& o) { return o.start; }
    // affine4_chain_kernel<false> over one chunk's jobs (the chained route's host side is affine_chain_host.hpp's)
    static bool launch_chain_run(const Batch& ab, const ChainJob* d_jobs, int njobs, const Pair* d_pairs, uint32_t* ticket_err, hipStream_t s) {
        const dim3 grid((njobs + kBlockWaves - 1) / kBlockWaves), block(64 * kBlockWaves);
        if (ab.free_ends)
            hipLaunchKernelGGL((affine4_chain_kernel<false, true>), grid, block, 0, s, d_jobs, njobs, d_pairs, ab.C, 0u, ticket_err, ab.d_cost.as<int32_t>(),
                               ends_of(ab));
        else
            hipLaunchKernelGGL((affine4_chain_kernel<false, false>), grid, block, 0, s, d_jobs, njobs, d_pairs, ab.C, 0u, ticket_err,
                               ab.d_cost.as<int32_t>(), Ends{});
        return hip_ok(hipGetLastError(), "affine4_chain_kernel launch");
    }
};

}  // namespace

extern "C" pa_affine4_batch* pa_affine4_batch_create(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b, const size_t* b_len,
                                                     size_t npairs, const pa_affine4_cost* cm, int trace) {
    if (!cm) {
        set_error("pa_affine4_batch_create: NULL cost model");
        return nullptr;
    }
    if (npairs && (!a || !a_len || !b || !b_len)) {
        set_error("pa_affine4_batch_create: NULL array");
        return nullptr;
    }
    // the cost model (AffineCost::new, cost_model.rs): every present cost >= 1, here also <= 1000; 0 = absent, for sub / ins / del only
    const int32_t lin[3] = {cm->sub, cm->ins, cm->del};
    static const char* names[3] = {"sub", "ins", "del"};
    for (int k = 0; k < 3; ++k)
        if (lin[k] < 0 || lin[k] > kMaxCost) {
            set_error("pa_affine4_batch_create: cost %s = %d outside [1, %d] (0 = absent)", names[k], lin[k], kMaxCost);
            return nullptr;
        }
    uint64_t max_edge = std::max({(uint64_t)cm->sub, (uint64_t)cm->ins, (uint64_t)cm->del});
    for (int k = 0; k < 4; ++k) {
        if (cm->open[k] < 1 || cm->open[k] > kMaxCost || cm->extend[k] < 1 || cm->extend[k] > kMaxCost) {
            set_error("pa_affine4_batch_create: layer %d (%s): open = %d, extend = %d outside [1, %d] (all four layers are required)", k,
                      k & 1 ? "delete" : "insert", cm->open[k], cm->extend[k], kMaxCost);
            return nullptr;
        }
        max_edge = std::max(max_edge, (uint64_t)cm->open[k] + (uint64_t)cm->extend[k]);
    }
    Costs C{};
    auto cost = [](int32_t c) { return c ? (uint32_t)c : kInf; };
    C.sub = cost(cm->sub);
    C.ins = cost(cm->ins);
    C.del = cost(cm->del);
    for (int k = 0; k < 4; ++k) {
        C.oe[k] = (uint32_t)cm->open[k] + (uint32_t)cm->extend[k];
        C.e[k] = (uint32_t)cm->extend[k];
    }
    return affine_host::create<Host>(a, a_len, b, b_len, npairs, trace, max_edge, C);
}

extern "C" int pa_affine4_batch_run(pa_affine4_batch* ab, int32_t* cost_out, float* kernel_ms) {
    if (!ab) return fail(PA_E_ARG, "pa_affine4_batch_run: NULL batch");
    if (kernel_ms) *kernel_ms = 0;
    hipStream_t s = 0;
    if (ab->np == 0) return Host::finish(*ab, cost_out, s);  // (nothing to copy: the call counts for pa_affine4_batch_ends)
    affine_host::Events ev;
    if (!ev.make()) return PA_E_HIP;
    affine_host::chain_begin(*ab);
    if (ab->chain.on && !ab->chain.ids.empty()) {  // the packed pairs' launch, then a wavefront per strip of the others
        if (const int rc = affine_host::run_chained<Host>(*ab, ev, s)) return rc;
    } else if (!hip_ok(hipEventRecord(ev.e[0], s), "event") || !Host::launch<false>(*ab, ab->fwd, s) || !hip_ok(hipEventRecord(ev.e[1], s), "event") ||
               !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    if (const int rc = Host::finish(*ab, cost_out, s)) return rc;
    if (kernel_ms && !hip_ok(hipEventElapsedTime(kernel_ms, ev.e[0], ev.e[1]), "hipEventElapsedTime")) return PA_E_HIP;
    return 0;
}

extern "C" int pa_affine4_batch_align(pa_affine4_batch* ab, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    return affine_host::align<Host>(ab, cost_out, cigar_out, forward_ms, trace_ms);
}

extern "C" void pa_affine4_batch_info(const pa_affine4_batch* ab, double* waves, double* packed_pairs, double* strip_pairs, double* lane_use,
                                      double* trace_chunks) {
    affine_host::batch_info(ab, waves, packed_pairs, strip_pairs, lane_use, trace_chunks);
}

extern "C" int pa_affine4_batch_set_chain(pa_affine4_batch* ab, int on) { return affine_host::set_chain<Host>(ab, on); }

extern "C" void pa_affine4_batch_chain_info(const pa_affine4_batch* ab, double* on, double* chain_pairs, double* chain_jobs, double* chunks,
                                            double* bnd_bytes_max) {
    affine_host::chain_info(ab, on, chain_pairs, chain_jobs, chunks, bnd_bytes_max);
}

extern "C" int pa_affine4_batch_set_free_ends(pa_affine4_batch* ab, int free_start, int free_end) {
    return affine_host::set_free_ends<Host>(ab, free_start, free_end);
}

extern "C" int pa_affine4_batch_ends(const pa_affine4_batch* ab, int64_t* start_out, int64_t* end_out) {
    return affine_host::batch_ends<Host>(ab, start_out, end_out);
}

extern "C" int pa_affine4_batch_last_row(pa_affine4_batch* ab, int32_t* out, const uint64_t* offsets) {
    return affine_host::last_row<Host>(ab, out, offsets);
}

extern "C" void pa_affine4_batch_destroy(pa_affine4_batch* ab) {
    if (!ab) return;
    (void)hipDeviceSynchronize();
    dt_release(ab->dt);
    delete ab;
}
