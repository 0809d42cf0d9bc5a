// affine4_dt_unit.hip -- the diagonal-transition (WFA) route of the batched double-affine aligner: pa_affine4_batch_run_dt, _align_dt,
// their ends-free forms _run_dt_ends and _align_dt_ends (the switches are arguments of the call), and _dt_info
// (include/pa_affine4_dt_hip.h).  Every pair gets a block of affine4_dt_kernel (affine4_dt_kernel.hpp), one wavefront or four, and a
// block of fronts in device memory whose size is known from s_max and the lengths (affine4_dt_plan.hpp): per-layer rings for run_dt,
// every front up to s_max for align_dt, which then walks them back on the GPU (affine4_dt_walk_kernel).  The pairs run most expensive
// first, in chunks whose fronts fit PA_AFFINE_TRACE_BUDGET_MB.  There is no retry: a pair whose cost exceeds s_max is reported as -1.
//
// The driver below restates affine_dt_unit.hip's dt_call (event timing, the chunk loop, the copy-back of the ops) over this unit's
// plan, job record and kernels; sharing it is left to a change that may touch that unit ("Double-affine diagonal
// transition").  The segmented traceback is affine4_dt_seg_unit.hip's; the state of both is affine4_dt_host.hpp's.
#include "pa_hip_internal.hpp"
#include "affine4_dt_kernel.hpp"
#include "affine4_dt_plan.hpp"
#include "affine4_dt_host.hpp"
#include "affine4_dt_view.hpp"
#include "../../include/pa_affine4_dt_hip.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace pa;
using namespace pa::affine4;

void pa::affine4::dt_release(DtState* st) { delete st; }

namespace {

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

using ForwardFn = void (*)(const dt::Job*, dt::Costs, int32_t*, dt::Stat*);
using WalkFn = void (*)(const dt::Job*, int, dt::Costs, const int32_t*, dt::WalkOut*);
ForwardFn forward_of(bool fs, bool fe) {
    return fs ? (fe ? dt::affine4_dt_kernel<true, true> : dt::affine4_dt_kernel<true, false>)
              : (fe ? dt::affine4_dt_kernel<false, true> : dt::affine4_dt_kernel<>);
}
WalkFn walk_of(bool fs, bool fe) {
    return fs ? (fe ? dt::affine4_dt_walk_kernel<true, true> : dt::affine4_dt_walk_kernel<true, false>)
              : (fe ? dt::affine4_dt_walk_kernel<false, true> : dt::affine4_dt_walk_kernel<>);
}

// One DT call.  own_ends: the call brings its switches (the _ends functions), and the batch's ends-free setting is not looked at; else
// the call is global and refuses a batch whose setting is on.  start_out / end_out: of the _ends functions (with both switches off
// start = 0 and end = |a|); -1 for a pair that was not found.
int dt_call(const char* fn, pa_affine4_batch* ab, bool own_ends, int free_start, int free_end, int32_t s_max, bool traced, int32_t* cost_out,
            int64_t* start_out, int64_t* end_out, std::vector<std::string>* cigars, float* fwd_ms, float* walk_ms) {
    const DtView v = dt_view(ab);
    if ((free_start | free_end) & ~1) return fail(PA_E_ARG, "%s: free_start = %d, free_end = %d: each is 0 or 1", fn, free_start, free_end);
    if (s_max < 0 || s_max >= kSMaxLimit) return fail(PA_E_ARG, "%s: s_max = %d outside [0, 2^30)", fn, s_max);
    if (!own_ends && v.ends) return fail(PA_E_ARG, "%s: the batch is in ends-free mode; %s_ends takes the switches as arguments", fn, fn);
    const bool fs = free_start != 0, fe = free_end != 0, ends = fs || fe;  // ends: the kernels keep {cost, end} per pair
    if (traced && !v.trace) return fail(PA_E_ARG, "%s: the batch was created without trace", fn);
    if (!*v.state) *v.state = new (std::nothrow) DtState;
    DtState* st = *v.state;
    if (!st) return fail(PA_E_NOMEM, "out of memory");
    st->found = st->not_found = st->chunks = st->front_cells = st->extend_chars = st->bytes_max = 0;
    if (v.np == 0) return 0;
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    const dt::Plan P = dt::plan(v.n, v.m, v.np, v.C, s_max, traced, fs, fe, budget);
    if (P.refused >= 0) {
        const dt::Shape& S = P.shape[(size_t)P.refused];
        return fail(PA_E_ARG, "%s: pair %lld: %zu bytes of fronts (s_max %d, %u diagonals) exceed the budget of %zu bytes", fn, P.refused, S.bytes,
                    S.s_max, S.W - 2, budget);
    }
    hipStream_t s = 0;
    if (!st->seq_ready) {
        if (!st->d_seq.alloc(v.seq_bytes + dt::kSeqPad) ||
            (v.seq_bytes && !hip_ok(hipMemcpyAsync(st->d_seq.ptr, v.d_seq, v.seq_bytes, hipMemcpyDeviceToDevice, s), "D2D")) ||
            !hip_ok(hipMemsetAsync(st->d_seq.as<uint8_t>() + v.seq_bytes, 0, dt::kSeqPad, s), "hipMemsetAsync"))
            return PA_E_HIP;
        st->seq_ready = true;
    }
    Events ev;
    const ForwardFn forward = forward_of(fs, fe);
    const WalkFn walk = walk_of(fs, fe);
    if (!ev.make() || !st->d_cost.reserve(v.np * (ends ? 8 : 4)) || !st->d_stat.reserve(v.np * sizeof(dt::Stat)) ||
        !hip_ok(hipMemsetAsync(st->d_stat.ptr, 0, v.np * sizeof(dt::Stat), s), "hipMemsetAsync"))
        return PA_E_HIP;
    float fwd_total = 0, walk_total = 0;
    std::vector<dt::Job> jobs;
    std::vector<dt::WalkOut> wout;
    std::vector<uint8_t> ops;
    for (const dt::Chunk& ch : P.chunks) {
        st->chunks += 1;
        st->bytes_max = std::max(st->bytes_max, (double)ch.bytes);
        if (!st->d_fronts.reserve(std::max<size_t>(ch.bytes, 16))) return PA_E_HIP;
        jobs.clear();
        for (size_t x = ch.first; x < ch.first + ch.count; ++x) {
            const uint32_t p = P.order[x];
            const dt::Shape& S = P.shape[p];
            dt::Job J;
            std::memset(&J, 0, sizeof J);
            J.a = st->d_seq.as<uint8_t>() + v.aoff[p];
            J.b = st->d_seq.as<uint8_t>() + v.boff[p];
            uint8_t* base = st->d_fronts.as<uint8_t>() + P.off[p];
            J.fronts = reinterpret_cast<int32_t*>(base);
            J.ops = traced ? base + (S.bytes - S.ops_bytes) : nullptr;
            J.n = S.n, J.m = S.m, J.s_max = S.s_max, J.W = S.W, J.kmin = S.kmin, J.kmax = S.kmax, J.out = p;
            for (int t = 0; t < 5; ++t) J.depth[t] = S.depth[t];
            jobs.push_back(J);
        }
        const int nj = (int)jobs.size();
        const int threads = ch.wide ? dt::kWideBlock : 64;  // four wavefronts to a pair where the chunk's fronts are wide
        if (!st->d_jobs.reserve(jobs.size() * sizeof(dt::Job)) ||
            !hip_ok(hipMemcpyAsync(st->d_jobs.ptr, jobs.data(), jobs.size() * sizeof(dt::Job), hipMemcpyHostToDevice, s), "H2D") ||
            !hip_ok(hipStreamSynchronize(s), "sync") ||  // (jobs is pageable memory, reused by the next chunk)
            !hip_ok(hipEventRecord(ev.e[0], s), "event") || !hip_ok(hipMemsetAsync(st->d_fronts.ptr, dt::kNegByte, ch.bytes, s), "hipMemsetAsync"))
            return PA_E_HIP;
        hipLaunchKernelGGL(forward, dim3(nj), dim3(threads), 0, s, st->d_jobs.as<dt::Job>(), v.C, st->d_cost.as<int32_t>(), st->d_stat.as<dt::Stat>());
        if (!hip_ok(hipGetLastError(), "affine4_dt_kernel launch") || !hip_ok(hipEventRecord(ev.e[1], s), "event")) return PA_E_HIP;
        if (traced) {
            if (!st->d_wout.reserve(jobs.size() * sizeof(dt::WalkOut))) return PA_E_HIP;
            hipLaunchKernelGGL(walk, dim3((nj + 63) / 64), dim3(64), 0, s, st->d_jobs.as<dt::Job>(), nj, v.C, st->d_cost.as<int32_t>(),
                               st->d_wout.as<dt::WalkOut>());
            wout.resize(jobs.size());
            if (!hip_ok(hipGetLastError(), "affine4_dt_walk_kernel launch") || !hip_ok(hipEventRecord(ev.e[2], s), "event") ||
                !hip_ok(hipMemcpyAsync(wout.data(), st->d_wout.ptr, jobs.size() * sizeof(dt::WalkOut), hipMemcpyDeviceToHost, s), "D2H") ||
                !hip_ok(hipStreamSynchronize(s), "sync"))
                return PA_E_HIP;
            std::vector<size_t> at(jobs.size() + 1, 0);  // every pair's ops lie behind its fronts: one copy per pair
            for (size_t x = 0; x < jobs.size(); ++x) {
                if (wout[x].status != 0)
                    return fail(PA_E_INTERNAL, "%s: pair %u: %s", fn, jobs[x].out, wout[x].status == 1 ? "a front holds no parent" : "path longer than its buffer");
                at[x + 1] = at[x] + (size_t)wout[x].nops;
            }
            ops.resize(at.back());
            for (size_t x = 0; x < jobs.size(); ++x)
                if (wout[x].nops && !hip_ok(hipMemcpyAsync(ops.data() + at[x], jobs[x].ops, (size_t)wout[x].nops, hipMemcpyDeviceToHost, s), "D2H"))
                    return PA_E_HIP;
            if (!hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
            for (size_t x = 0; x < jobs.size(); ++x) {
                (*cigars)[jobs[x].out] = cigar_of(ops.data() + at[x], wout[x].nops);
                if (start_out)  // the bytes of a the path consumes (every op but an insertion's): start = end - these
                    start_out[jobs[x].out] = (int64_t)std::count_if(ops.data() + at[x], ops.data() + at[x + 1],
                                                                    [](uint8_t op) { return op != 'I' && op != 'i' && op != 'j'; });
            }
            float t = 0;
            if (!hip_ok(hipEventElapsedTime(&t, ev.e[1], ev.e[2]), "hipEventElapsedTime")) return PA_E_HIP;
            walk_total += t;
        } else if (!hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        float f = 0;
        if (!hip_ok(hipEventElapsedTime(&f, ev.e[0], ev.e[1]), "hipEventElapsedTime")) return PA_E_HIP;
        fwd_total += f;
    }
    std::vector<int32_t> cost(v.np * (ends ? 2 : 1));
    std::vector<dt::Stat> stat(v.np);
    if (!hip_ok(hipMemcpyAsync(cost.data(), st->d_cost.ptr, cost.size() * 4, hipMemcpyDeviceToHost, s), "D2H") ||
        !hip_ok(hipMemcpyAsync(stat.data(), st->d_stat.ptr, v.np * sizeof(dt::Stat), hipMemcpyDeviceToHost, s), "D2H") ||
        !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    for (size_t p = 0; p < v.np; ++p) {
        const int64_t end = cost[ends ? 2 * p : p] < 0 ? -1 : ends ? cost[2 * p + 1] : (int64_t)v.n[p];
        if (ends) cost[p] = cost[2 * p];
        if (end_out) end_out[p] = end;
        if (start_out) start_out[p] = end < 0 ? -1 : end - start_out[p];
        (cost[p] >= 0 ? st->found : st->not_found) += 1;
        st->front_cells += (double)stat[p].front_cells;
        st->extend_chars += (double)stat[p].extend_chars;
    }
    if (cost_out) std::memcpy(cost_out, cost.data(), v.np * 4);
    if (fwd_ms) *fwd_ms = fwd_total;
    if (walk_ms) *walk_ms = walk_total;
    return 0;
}

}  // namespace

extern "C" int pa_affine4_batch_run_dt(pa_affine4_batch* ab, int32_t s_max, int32_t* cost_out, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine4_batch_run_dt: NULL batch");
    return dt_call("pa_affine4_batch_run_dt", ab, false, 0, 0, s_max, false, cost_out, nullptr, nullptr, nullptr, kernel_ms, nullptr);
}

extern "C" int pa_affine4_batch_run_dt_ends(pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, int64_t* end_out,
                                            float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine4_batch_run_dt_ends: NULL batch");
    return dt_call("pa_affine4_batch_run_dt_ends", ab, true, free_start, free_end, s_max, false, cost_out, nullptr, end_out, nullptr, kernel_ms, nullptr);
}

extern "C" int pa_affine4_batch_align_dt(pa_affine4_batch* ab, int32_t s_max, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    if (forward_ms) *forward_ms = 0;
    if (trace_ms) *trace_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine4_batch_align_dt: NULL batch");
    const size_t np = dt_view(ab).np;
    if (cigar_out)
        for (size_t p = 0; p < np; ++p) cigar_out[p] = nullptr;
    std::vector<std::string> cigars(np);
    if (const int rc = dt_call("pa_affine4_batch_align_dt", ab, false, 0, 0, s_max, true, cost_out, nullptr, nullptr, &cigars, forward_ms, trace_ms))
        return rc;
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" int pa_affine4_batch_align_dt_ends(pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, int64_t* start_out,
                                              int64_t* end_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    if (forward_ms) *forward_ms = 0;
    if (trace_ms) *trace_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine4_batch_align_dt_ends: NULL batch");
    const size_t np = dt_view(ab).np;
    if (cigar_out)
        for (size_t p = 0; p < np; ++p) cigar_out[p] = nullptr;
    std::vector<std::string> cigars(np);
    std::vector<int64_t> start(np);  // (dt_call counts the path's bytes of a here before it knows the ends)
    if (const int rc = dt_call("pa_affine4_batch_align_dt_ends", ab, true, free_start, free_end, s_max, true, cost_out, start.data(), end_out, &cigars,
                               forward_ms, trace_ms))
        return rc;
    if (start_out) std::copy(start.begin(), start.end(), start_out);
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" void pa_affine4_batch_dt_info(const pa_affine4_batch* ab, double* found, double* not_found, double* chunks, double* front_cells,
                                         double* extend_chars, double* bytes_max) {
    const DtState* st = ab ? *dt_view(const_cast<pa_affine4_batch*>(ab)).state : nullptr;
    if (found) *found = st ? st->found : 0;
    if (not_found) *not_found = st ? st->not_found : 0;
    if (chunks) *chunks = st ? st->chunks : 0;
    if (front_cells) *front_cells = st ? st->front_cells : 0;
    if (extend_chars) *extend_chars = st ? st->extend_chars : 0;
    if (bytes_max) *bytes_max = st ? st->bytes_max : 0;
}
