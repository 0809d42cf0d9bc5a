// affine4_local_unit.hip -- local (Smith-Waterman) alignment over a double-affine batch (pa_affine4_batch_run_local, _align_local,
// _local_info: include/pa_affine4_local_hip.h).  The four-layer counterpart of affine_local_unit.hip.
//
// The batch is affine4_batch.hpp's: of it this unit reads the pairs, the uploaded sequences, the cost model, the planner's order and
// the plan of run().  run_local() launches affine4_local_kernel<false> over that plan as it is.  align_local() re-runs the pairs with
// affine4_local_kernel<true> in chunks whose traceback codes fit the budget -- affine_host.hpp's chunks and plans, as align() has them
// -- and walks every pair's codes on the GPU (affine4_local_walk_kernel) from the end the fill left.  `match` comes with the call;
// nothing of the batch but the shape of the last align_local() (LocalInfo) is written, and the results live in buffers of the call's
// own, so no other route's state or results move: d_cost, d_end, free_ends, the chain state, the DT state and what
// pa_affine4_batch_ends reports are neither read nor written.
#include "affine4_local_kernel.hpp"
#include "affine4_batch.hpp"
#include "affine_host.hpp"
#include "../../include/pa_affine4_local_hip.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace pa;
using namespace pa::affine4;

namespace {

constexpr int32_t kMaxMatch = 1000;

using Plan = affine_host::Plan<Pair, Wave>;
using affine_host::Events;

// The checks every call starts with, then the costs of the step.
int begin(const char* fn, const pa_affine4_batch* ab, int32_t match, LocalCosts& C) {
    if (!ab) return fail(PA_E_ARG, "%s: NULL batch", fn);
    if (match < 1 || match > kMaxMatch) return fail(PA_E_ARG, "%s: match = %d outside [1, %d]", fn, match, kMaxMatch);
    for (size_t p = 0; p < ab->np; ++p) {
        const uint64_t top = (uint64_t)match * std::min(ab->n[p], ab->m[p]);
        if (top >= (uint64_t(1) << 30))
            return fail(PA_E_ARG, "%s: pair %zu: match * min(|a|, |b|) = %d * %u is not below 2^30", fn, p, match, std::min(ab->n[p], ab->m[p]));
    }
    auto edge = [](uint32_t c) { return c == kInf ? kLocalNoEdge : (int32_t)c; };
    C = LocalCosts{match, edge(ab->C.sub), edge(ab->C.ins), edge(ab->C.del), {}, {}};
    for (int k = 0; k < 4; ++k) {
        C.oe[k] = (int32_t)ab->C.oe[k];
        C.e[k] = (int32_t)ab->C.e[k];
    }
    return 0;
}

template <bool FILL>
bool launch(const Plan& P, const LocalCosts& C, int32_t* d_res, hipStream_t s) {
    const size_t nwaves = P.waves.size();
    if (nwaves == 0) return true;
    const int grid = (int)((nwaves + kBlockWaves - 1) / kBlockWaves);
    hipLaunchKernelGGL((affine4_local_kernel<FILL>), dim3(grid), dim3(64 * kBlockWaves), 0, s, P.d_waves.as<Wave>(), (int)nwaves, P.d_pairs.as<Pair>(), C,
                       d_res);
    return hip_ok(hipGetLastError(), FILL ? "affine4_local_kernel<FILL> launch" : "affine4_local_kernel launch");
}

// (score, a_end, b_end) of every pair from the device, to whichever outputs the caller gave.
int results_out(size_t np, const int32_t* d_res, int32_t* score_out, int64_t* a_end_out, int64_t* b_end_out, hipStream_t s) {
    std::vector<int32_t> res(np * 3);
    if (!hip_ok(hipMemcpyAsync(res.data(), d_res, res.size() * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    for (size_t p = 0; p < np; ++p) {
        if (score_out) score_out[p] = res[3 * p];
        if (a_end_out) a_end_out[p] = res[3 * p + 1];
        if (b_end_out) b_end_out[p] = res[3 * p + 2];
    }
    return 0;
}

}  // namespace

extern "C" int pa_affine4_batch_run_local(pa_affine4_batch* ab, int32_t match, int32_t* score_out, int64_t* a_end_out, int64_t* b_end_out,
                                          float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0;
    LocalCosts C;
    if (const int rc = begin("pa_affine4_batch_run_local", ab, match, C)) return rc;
    if (ab->np == 0) return 0;
    hipStream_t s = 0;
    DeviceBuf d_res;
    Events ev;
    if (!d_res.alloc(ab->np * 12) || !ev.make() || !hip_ok(hipEventRecord(ev.e[0], s), "event") || !launch<false>(ab->fwd, C, d_res.as<int32_t>(), s) ||
        !hip_ok(hipEventRecord(ev.e[1], s), "event"))
        return PA_E_HIP;
    if (const int rc = results_out(ab->np, d_res.as<int32_t>(), score_out, a_end_out, b_end_out, s)) return rc;
    if (kernel_ms && !hip_ok(hipEventElapsedTime(kernel_ms, ev.e[0], ev.e[1]), "hipEventElapsedTime")) return PA_E_HIP;
    return 0;
}

extern "C" int pa_affine4_batch_align_local(pa_affine4_batch* ab, int32_t match, int32_t* score_out, int64_t* a_start_out, int64_t* a_end_out,
                                            int64_t* b_start_out, int64_t* b_end_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    static const char* fn = "pa_affine4_batch_align_local";
    using Host = HostBase;
    if (forward_ms) *forward_ms = 0;
    if (trace_ms) *trace_ms = 0;
    LocalCosts C;
    if (ab && cigar_out)
        for (size_t p = 0; p < ab->np; ++p) cigar_out[p] = nullptr;
    if (const int rc = begin(fn, ab, match, C)) return rc;
    if (!ab->trace) return fail(PA_E_ARG, "%s: the batch was created without trace", fn);
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");  // (the traceback codes dominate a chunk)
    auto code_bytes = [&](uint32_t p) { return affine_plan::code_bytes_of(Host::kLayout, ab->n[p], ab->m[p]); };
    for (size_t p = 0; p < ab->np; ++p)
        if (code_bytes((uint32_t)p) > budget)
            return fail(PA_E_ARG, "%s: pair %zu: %zu bytes of traceback codes exceed the budget of %zu bytes", fn, p, code_bytes((uint32_t)p), budget);
    ab->local = LocalInfo{};
    const size_t np = ab->np;
    if (np == 0) return 0;
    hipStream_t s = 0;
    std::vector<std::string> cigars(np);
    std::vector<int64_t> a_start(np, 0), b_start(np, 0);
    float fwd_total = 0, trace_total = 0;
    DeviceBuf d_res, d_codes, d_ops, d_walk, d_wout;
    if (!d_res.alloc(np * 12)) return PA_E_HIP;
    for (size_t c0 = 0, bytes; c0 < np;) {
        const std::vector<uint32_t> ids = affine_plan::next_chunk(ab->order, c0, budget, code_bytes, &bytes);
        ab->local.chunks += 1;
        ab->local.bytes_max = std::max(ab->local.bytes_max, (double)bytes);
        if (!d_codes.reserve(std::max<size_t>(bytes, 16))) return PA_E_HIP;
        Plan P;
        if (const int rc = affine_host::make_plan<Host>(*ab, ids, P, affine_plan::Keep::kCodes, d_codes.as<uint8_t>(), s)) return rc;
        std::vector<Walk> walks(P.pairs.size());
        const size_t ops_bytes = P.at.ops_bytes;
        if (!d_ops.reserve(std::max<size_t>(ops_bytes, 16))) return PA_E_HIP;
        for (size_t k = 0; k < P.pairs.size(); ++k) {
            const Pair& Q = P.pairs[k];
            Walk& w = walks[k];
            w.a = Q.a;
            w.b = Q.b;
            w.codes = Q.codes;
            w.ops = d_ops.as<uint8_t>() + P.at.pairs[k].ops_off;
            w.n = Q.n;
            w.m = Q.m;
            w.H = Q.H;
            w.cap = Q.n + Q.m;
            w.out = Q.out;
            w.pad_ = 0;
        }
        const int nw = (int)walks.size();
        Events ev;
        if (!ev.make() || !upload(d_walk, walks.data(), walks.size() * sizeof(Walk), s) ||
            !d_wout.reserve(std::max<size_t>(nw * sizeof(LocalWalkOut), 16)) || !hip_ok(hipEventRecord(ev.e[0], s), "event") ||
            !launch<true>(P, C, d_res.as<int32_t>(), s) || !hip_ok(hipEventRecord(ev.e[1], s), "event"))
            return PA_E_HIP;
        std::vector<LocalWalkOut> wout(nw);
        std::vector<uint8_t> ops(ops_bytes);
        hipLaunchKernelGGL(affine4_local_walk_kernel, dim3((nw + 63) / 64), dim3(64), 0, s, d_walk.as<Walk>(), nw, d_wout.as<LocalWalkOut>(),
                           d_res.as<int32_t>());
        if (!hip_ok(hipGetLastError(), "affine4_local_walk_kernel launch") || !hip_ok(hipEventRecord(ev.e[2], s), "event") ||
            !hip_ok(hipMemcpyAsync(wout.data(), d_wout.ptr, nw * sizeof(LocalWalkOut), hipMemcpyDeviceToHost, s), "D2H") ||
            (ops_bytes && !hip_ok(hipMemcpyAsync(ops.data(), d_ops.ptr, ops_bytes, hipMemcpyDeviceToHost, s), "D2H")) ||
            !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        float f = 0, t = 0;
        if (!hip_ok(hipEventElapsedTime(&f, ev.e[0], ev.e[1]), "hipEventElapsedTime") || !hip_ok(hipEventElapsedTime(&t, ev.e[1], ev.e[2]), "hipEventElapsedTime"))
            return PA_E_HIP;
        fwd_total += f;
        trace_total += t;
        for (size_t k = 0; k < P.pairs.size(); ++k) {
            const LocalWalkOut& o = wout[k];
            const uint32_t p = P.pairs[k].out;
            if (o.status != 0) return fail(PA_E_INTERNAL, "%s: pair %u: %s", fn, p, o.status == 1 ? "bad traceback code" : "path longer than its buffer");
            cigars[p] = Host::cigar_of(ops.data() + P.at.pairs[k].ops_off, o.nops);
            a_start[p] = o.a_start;
            b_start[p] = o.b_start;
        }
        c0 += ids.size();
    }
    if (const int rc = results_out(np, d_res.as<int32_t>(), score_out, a_end_out, b_end_out, s)) return rc;
    if (a_start_out) std::memcpy(a_start_out, a_start.data(), np * 8);
    if (b_start_out) std::memcpy(b_start_out, b_start.data(), np * 8);
    if (forward_ms) *forward_ms = fwd_total;
    if (trace_ms) *trace_ms = trace_total;
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" void pa_affine4_batch_local_info(const pa_affine4_batch* ab, double* chunks, double* bytes_max) {
    const LocalInfo I = ab ? ab->local : LocalInfo{};
    if (chunks) *chunks = I.chunks;
    if (bytes_max) *bytes_max = I.bytes_max;
}
