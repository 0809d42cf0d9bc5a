// affine_dt_unit.hip -- the diagonal-transition (WFA) route of the batched gap-affine aligner: pa_affine_batch_run_dt, _align_dt, their
// ends-free forms _run_dt_ends and _align_dt_ends (the switches are arguments of the call), and _dt_info (include/pa_affine_hip.h).
// Every pair gets a block of affine_dt_kernel (affine_dt_kernel.hpp), one wavefront or four, and a block of fronts in device memory whose size is known from s_max and the lengths: a ring of `max edge + 1` fronts for run_dt, every front up to
// s_max for align_dt, which then walks them back on the GPU (affine_dt_walk_kernel).  The pairs run most expensive first, in chunks whose
// fronts fit PA_AFFINE_TRACE_BUDGET_MB.  There is no retry: a pair whose cost exceeds s_max is reported as -1.
#include "pa_hip_internal.hpp"
#include "engine.hpp"
#include "affine_dt_kernel.hpp"
#include "affine_dt_view.hpp"
#include "../../include/pa_affine_hip.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace pa;
using namespace pa::affine;

struct pa::affine::DtState {
    DeviceBuf d_seq;  // the batch's sequences, with kSeqPad bytes after the last
    bool seq_ready = false;
    DeviceBuf d_cost, d_stat, d_jobs, d_fronts, d_ops, d_wout;
    double found = 0, not_found = 0, chunks = 0, front_cells = 0, extend_chars = 0, bytes_max = 0;  // the last DT call
};

void pa::affine::dt_release(DtState* st) { delete st; }

namespace {

constexpr int32_t kSMaxLimit = 1 << 30;

uint64_t gap_cost(uint64_t L, uint32_t lin, uint32_t op, uint32_t ex) {
    if (L == 0) return 0;
    uint64_t c = UINT64_MAX;
    if (lin != kDtAbsent) c = L * lin;
    if (op != kDtAbsent) c = std::min<uint64_t>(c, op + L * ex);
    return c;
}
// The longest gap cost s pays for on any layer: s / lin on the main layer, (s - open) / extend + 1 on the affine one.
uint32_t reach(uint32_t s, uint32_t lin, uint32_t op, uint32_t ex) {
    uint32_t r = lin != kDtAbsent ? s / lin : 0;
    if (op != kDtAbsent && s >= op) r = std::max(r, (s - op) / ex + 1);
    return r;
}
bool has_layers(const DtCosts& C) { return C.io != kDtAbsent || C.dopen != kDtAbsent; }
uint32_t max_edge(const DtCosts& C) {
    uint32_t e = 0;
    for (const uint32_t c : {C.sub, C.ins, C.del, C.io, C.ie, C.dopen, C.de})
        if (c != kDtAbsent) e = std::max(e, c);
    return e;
}

// Pair p's job, but for its pointers, and the device bytes of its fronts (and ops).  Ends-free: inserting b is always a path (end = 0, or
// start = |a|), and under free_start the diagonals up to kmax are live from cost 0 on.  kmax = min(|a|, |a| - |b| + reach_ins(s')): a
// path through a diagonal above that needs more insertions than s' pays for to come back to an end diagonal (<= |a| - |b|), so no path
// within s' passes there and the results are those of kmax = |a|.  W = kmax + reach_ins(s') + 3, at most |a| + reach_ins(s') + 3.
dt::Job shape_of(const DtView& v, uint32_t p, int32_t s_max, bool traced, bool fs, bool fe, size_t* bytes) {
    dt::Job J;
    std::memset(&J, 0, sizeof J);
    const DtCosts& C = v.C;
    J.n = v.n[p];
    J.m = v.m[p];
    J.out = p;
    J.s_max = (int32_t)std::min<uint64_t>((uint64_t)s_max, (fs || fe ? 0 : gap_cost(J.n, C.del, C.dopen, C.de)) + gap_cost(J.m, C.ins, C.io, C.ie));
    const uint32_t back = reach((uint32_t)J.s_max, C.ins, C.io, C.ie);
    J.kmin = -(int32_t)std::min(J.m, back);
    J.kmax = fs ? (int32_t)std::min<int64_t>(J.n, std::max<int64_t>(0, (int64_t)J.n - (int64_t)J.m + back))
                : (int32_t)std::min(J.n, reach((uint32_t)J.s_max, C.del, C.dopen, C.de));
    J.W = (uint32_t)(J.kmax - J.kmin + 3);
    J.nslots = traced ? (uint32_t)J.s_max + 1 : max_edge(C) + 1;
    *bytes = ((size_t)J.nslots + 1) * (has_layers(C) ? 3 : 1) * J.W * 4 + (traced ? (((size_t)J.n + J.m + 15) & ~size_t(15)) : 0);
    return J;
}

std::string cigar_of(const uint8_t* op, int32_t nops) {  // the ops run from the end backwards
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

using ForwardFn = void (*)(const dt::Job*, DtCosts, int32_t*, dt::Stat*);
using WalkFn = void (*)(const dt::Job*, int, DtCosts, const int32_t*, dt::WalkOut*);
template <bool AFF>
ForwardFn forward_of(bool fs, bool fe) {
    return fs ? (fe ? dt::affine_dt_kernel<AFF, true, true> : dt::affine_dt_kernel<AFF, true, false>)
              : (fe ? dt::affine_dt_kernel<AFF, false, true> : dt::affine_dt_kernel<AFF>);
}
template <bool AFF>
WalkFn walk_of(bool fs, bool fe) {
    return fs ? (fe ? dt::affine_dt_walk_kernel<AFF, true, true> : dt::affine_dt_walk_kernel<AFF, true, false>)
              : (fe ? dt::affine_dt_walk_kernel<AFF, false, true> : dt::affine_dt_walk_kernel<AFF>);
}

// One DT call.  own_ends: the call brings its switches (the _ends functions), and the batch's ends-free setting is not looked at; else
// the call is global and refuses a batch whose setting is on.  start_out / end_out: of the _ends functions (with both switches off
// start = 0 and end = |a|); -1 for a pair that was not found.
int dt_call(const char* fn, pa_affine_batch* ab, bool own_ends, int free_start, int free_end, int32_t s_max, bool traced, int32_t* cost_out,
            int64_t* start_out, int64_t* end_out, std::vector<std::string>* cigars, float* fwd_ms, float* walk_ms) {
    const DtView v = dt_view(ab);
    if ((free_start | free_end) & ~1) return fail(PA_E_ARG, "%s: free_start = %d, free_end = %d: each is 0 or 1", fn, free_start, free_end);
    if (s_max < 0 || s_max >= kSMaxLimit) return fail(PA_E_ARG, "%s: s_max = %d outside [0, 2^30)", fn, s_max);
    if (!own_ends && v.C.ends) return fail(PA_E_ARG, "%s: the diagonal-transition route has no ends-free mode", fn);
    const bool fs = free_start != 0, fe = free_end != 0, ends = fs || fe;  // ends: the kernels keep {cost, end} per pair
    if (traced && !v.trace) return fail(PA_E_ARG, "%s: the batch was created without trace", fn);
    if (!*v.state) *v.state = new (std::nothrow) DtState;
    DtState* st = *v.state;
    if (!st) return fail(PA_E_NOMEM, "out of memory");
    st->found = st->not_found = st->chunks = st->front_cells = st->extend_chars = st->bytes_max = 0;
    if (v.np == 0) return 0;
    hipStream_t s = 0;
    if (!st->seq_ready) {
        if (!st->d_seq.alloc(v.seq_bytes + dt::kSeqPad) ||
            (v.seq_bytes && !hip_ok(hipMemcpyAsync(st->d_seq.ptr, v.d_seq, v.seq_bytes, hipMemcpyDeviceToDevice, s), "D2D")) ||
            !hip_ok(hipMemsetAsync(st->d_seq.as<uint8_t>() + v.seq_bytes, 0, dt::kSeqPad, s), "hipMemsetAsync"))
            return PA_E_HIP;
        st->seq_ready = true;
    }
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    std::vector<dt::Job> shape(v.np);
    std::vector<size_t> bytes(v.np);
    for (size_t p = 0; p < v.np; ++p) {
        shape[p] = shape_of(v, (uint32_t)p, s_max, traced, fs, fe, &bytes[p]);
        if (bytes[p] > budget)
            return fail(PA_E_ARG, "%s: pair %zu: %zu bytes of fronts (s_max %d, %u diagonals) exceed the budget of %zu bytes", fn, p, bytes[p],
                        shape[p].s_max, shape[p].W - 2, budget);
    }
    // most expensive first: cost steps x diagonals
    std::vector<uint32_t> order(v.np);
    for (size_t p = 0; p < v.np; ++p) order[p] = (uint32_t)p;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return ((uint64_t)shape[x].s_max + 1) * shape[x].W > ((uint64_t)shape[y].s_max + 1) * shape[y].W;
    });
    const bool aff = has_layers(v.C);
    Events ev;
    const ForwardFn forward = aff ? forward_of<true>(fs, fe) : forward_of<false>(fs, fe);
    const WalkFn walk = aff ? walk_of<true>(fs, fe) : walk_of<false>(fs, fe);
    if (!ev.make() || !st->d_cost.reserve(v.np * (ends ? 8 : 4)) || !st->d_stat.reserve(v.np * sizeof(dt::Stat)) ||
        !hip_ok(hipMemsetAsync(st->d_stat.ptr, 0, v.np * sizeof(dt::Stat), s), "hipMemsetAsync"))
        return PA_E_HIP;
    float fwd_total = 0, walk_total = 0;
    std::vector<dt::Job> jobs;
    std::vector<dt::WalkOut> wout;
    std::vector<uint8_t> ops;
    for (size_t c0 = 0; c0 < v.np;) {
        size_t c1 = c0, total = 0;
        while (c1 < v.np && (c1 == c0 || total + bytes[order[c1]] <= budget)) total += bytes[order[c1]], ++c1;
        st->chunks += 1;
        st->bytes_max = std::max(st->bytes_max, (double)total);
        if (!st->d_fronts.reserve(std::max<size_t>(total, 16))) return PA_E_HIP;
        jobs.clear();
        size_t off = 0;
        for (size_t x = c0; x < c1; ++x) {
            dt::Job J = shape[order[x]];
            J.a = st->d_seq.as<uint8_t>() + v.aoff[J.out];
            J.b = st->d_seq.as<uint8_t>() + v.boff[J.out];
            uint8_t* base = st->d_fronts.as<uint8_t>() + off;
            const size_t ops_bytes = traced ? (((size_t)J.n + J.m + 15) & ~size_t(15)) : 0;
            J.fronts = reinterpret_cast<int32_t*>(base);
            J.ops = traced ? base + (bytes[J.out] - ops_bytes) : nullptr;
            off += bytes[J.out];
            jobs.push_back(J);
        }
        const int nj = (int)jobs.size();
        // four wavefronts to a pair where the chunk's fronts are wide (a few rounds of 256 diagonals per step instead of many of 64)
        double wsum = 0;
        for (const dt::Job& J : jobs) wsum += J.W;
        const int threads = wsum / nj > dt::kWideMean ? dt::kWideBlock : 64;
        if (!st->d_jobs.reserve(jobs.size() * sizeof(dt::Job)) ||
            !hip_ok(hipMemcpyAsync(st->d_jobs.ptr, jobs.data(), jobs.size() * sizeof(dt::Job), hipMemcpyHostToDevice, s), "H2D") ||
            !hip_ok(hipStreamSynchronize(s), "sync") ||  // (jobs is pageable memory, reused by the next chunk)
            !hip_ok(hipEventRecord(ev.e[0], s), "event") || !hip_ok(hipMemsetAsync(st->d_fronts.ptr, dt::kNegByte, total, s), "hipMemsetAsync"))
            return PA_E_HIP;
        hipLaunchKernelGGL(forward, dim3(nj), dim3(threads), 0, s, st->d_jobs.as<dt::Job>(), v.C, st->d_cost.as<int32_t>(), st->d_stat.as<dt::Stat>());
        if (!hip_ok(hipGetLastError(), "affine_dt_kernel launch") || !hip_ok(hipEventRecord(ev.e[1], s), "event")) return PA_E_HIP;
        if (traced) {
            if (!st->d_wout.reserve(jobs.size() * sizeof(dt::WalkOut))) return PA_E_HIP;
            hipLaunchKernelGGL(walk, dim3((nj + 63) / 64), dim3(64), 0, s, st->d_jobs.as<dt::Job>(), nj, v.C, st->d_cost.as<int32_t>(),
                               st->d_wout.as<dt::WalkOut>());
            wout.resize(jobs.size());
            if (!hip_ok(hipGetLastError(), "affine_dt_walk_kernel launch") || !hip_ok(hipEventRecord(ev.e[2], s), "event") ||
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
                if (start_out)  // the bytes of a the path consumes: start = end - these
                    start_out[jobs[x].out] = (int64_t)std::count_if(ops.data() + at[x], ops.data() + at[x + 1], [](uint8_t op) { return op != 'I'; });
            }
            float t = 0;
            if (!hip_ok(hipEventElapsedTime(&t, ev.e[1], ev.e[2]), "hipEventElapsedTime")) return PA_E_HIP;
            walk_total += t;
        } else if (!hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        float f = 0;
        if (!hip_ok(hipEventElapsedTime(&f, ev.e[0], ev.e[1]), "hipEventElapsedTime")) return PA_E_HIP;
        fwd_total += f;
        c0 = c1;
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

extern "C" int pa_affine_batch_run_dt(pa_affine_batch* ab, int32_t s_max, int32_t* cost_out, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_run_dt: NULL batch");
    return dt_call("pa_affine_batch_run_dt", ab, false, 0, 0, s_max, false, cost_out, nullptr, nullptr, nullptr, kernel_ms, nullptr);
}

extern "C" int pa_affine_batch_run_dt_ends(pa_affine_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, int64_t* end_out,
                                           float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_run_dt_ends: NULL batch");
    return dt_call("pa_affine_batch_run_dt_ends", ab, true, free_start, free_end, s_max, false, cost_out, nullptr, end_out, nullptr, kernel_ms, nullptr);
}

extern "C" int pa_affine_batch_align_dt(pa_affine_batch* ab, int32_t s_max, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    if (forward_ms) *forward_ms = 0;
    if (trace_ms) *trace_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_align_dt: NULL batch");
    const size_t np = dt_view(ab).np;
    if (cigar_out)
        for (size_t p = 0; p < np; ++p) cigar_out[p] = nullptr;
    std::vector<std::string> cigars(np);
    if (const int rc = dt_call("pa_affine_batch_align_dt", ab, false, 0, 0, s_max, true, cost_out, nullptr, nullptr, &cigars, forward_ms, trace_ms))
        return rc;
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" int pa_affine_batch_align_dt_ends(pa_affine_batch* ab, int free_start, int free_end, int32_t s_max, int32_t* cost_out, int64_t* start_out,
                                             int64_t* end_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    if (forward_ms) *forward_ms = 0;
    if (trace_ms) *trace_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_align_dt_ends: NULL batch");
    const size_t np = dt_view(ab).np;
    if (cigar_out)
        for (size_t p = 0; p < np; ++p) cigar_out[p] = nullptr;
    std::vector<std::string> cigars(np);
    std::vector<int64_t> start(np);  // (dt_call counts the path's bytes of a here before it knows the ends)
    if (const int rc = dt_call("pa_affine_batch_align_dt_ends", ab, true, free_start, free_end, s_max, true, cost_out, start.data(), end_out, &cigars,
                               forward_ms, trace_ms))
        return rc;
    if (start_out) std::copy(start.begin(), start.end(), start_out);
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" void pa_affine_batch_dt_info(const pa_affine_batch* ab, double* found, double* not_found, double* chunks, double* front_cells,
                                        double* extend_chars, double* bytes_max) {
    const DtState* st = ab ? *dt_view(const_cast<pa_affine_batch*>(ab)).state : nullptr;
    if (found) *found = st ? st->found : 0;
    if (not_found) *not_found = st ? st->not_found : 0;
    if (chunks) *chunks = st ? st->chunks : 0;
    if (front_cells) *front_cells = st ? st->front_cells : 0;
    if (extend_chars) *extend_chars = st ? st->extend_chars : 0;
    if (bytes_max) *bytes_max = st ? st->bytes_max : 0;
}
