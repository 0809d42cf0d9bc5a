// affine_dt_unit.hip -- the diagonal-transition (WFA) route of the batched gap-affine aligner: pa_affine_batch_run_dt, _align_dt, their
// ends-free forms _run_dt_ends and _align_dt_ends (the switches are arguments of the call), and _dt_info (include/pa_affine_hip.h).
// Every pair gets a block of affine_dt_kernel (affine_dt_kernel.hpp), one wavefront or four, and a block of fronts in device memory whose size is known from s_max and the lengths: a ring of `max edge + 1` fronts for run_dt, every front up to
// s_max for align_dt, which then walks them back on the GPU (affine_dt_walk_kernel).  The pairs run most expensive first, in chunks whose
// fronts fit PA_AFFINE_TRACE_BUDGET_MB.  There is no retry: a pair whose cost exceeds s_max is reported as -1.
// pa_affine_batch_align_dt_seg traces in bounded memory instead (affine_dt_seg_kernel.hpp): a checkpointing pass over the ring, then per
// round one launch that re-fills a segment of fronts for every unfinished pair and one that walks it; _dt_seg_info reports its shape.
#include "pa_hip_internal.hpp"
#include "engine.hpp"
#include "affine_dt_kernel.hpp"
#include "affine_dt_seg_kernel.hpp"
#include "affine_dt_view.hpp"
#include "../../include/pa_affine_hip.h"

#include <algorithm>
#include <cmath>
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
    DeviceBuf d_seg_jobs, d_seg_state, d_seg_stat;
    double seg_chunks = 0, seg_rounds = 0, seg_jobs = 0, seg_refill_cells = 0, seg_bytes_max = 0;  // the last align_dt_seg
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


// ---- the segmented traceback (affine_dt_seg_kernel.hpp) ----

using CkptFn = void (*)(const dt::CkJob*, DtCosts, int32_t*, dt::Stat*);
using FillFn = void (*)(const dt::SegJob*, DtCosts, dt::Stat*);
using SegWalkFn = void (*)(const dt::SegJob*, int, DtCosts, dt::WalkState*);
template <bool AFF>
CkptFn ckpt_of(bool fs, bool fe) {
    return fs ? (fe ? dt::affine_dt_ckpt_kernel<AFF, true, true> : dt::affine_dt_ckpt_kernel<AFF, true, false>)
              : (fe ? dt::affine_dt_ckpt_kernel<AFF, false, true> : dt::affine_dt_ckpt_kernel<AFF>);
}
template <bool AFF>
SegWalkFn seg_walk_of(bool fs, bool fe) {
    return fs ? (fe ? dt::affine_dt_seg_walk_kernel<AFF, true, true> : dt::affine_dt_seg_walk_kernel<AFF, true, false>)
              : (fe ? dt::affine_dt_seg_walk_kernel<AFF, false, true> : dt::affine_dt_seg_walk_kernel<AFF>);
}

// Pair p under the segmented route: the ring job, the segment length, the segments that get checkpoint rows, and the device bytes of
// each part (include/pa_affine_hip.h states the sum).
struct SegShape {
    dt::Job j;
    uint32_t S, nck;
    size_t ring, ck, buf, ops, bytes;
};

constexpr size_t kSegPairState = sizeof(dt::WalkState) + sizeof(dt::Stat);  // per pair, outside the fronts: the walk state and the fills' counters

uint32_t ceil_sqrt(uint64_t x) {
    uint64_t r = (uint64_t)std::sqrt((double)x);
    while (r * r < x) ++r;
    while (r && (r - 1) * (r - 1) >= x) --r;
    return (uint32_t)r;
}

SegShape seg_shape_of(const DtView& v, uint32_t p, int32_t s_max, uint32_t seg, bool fs, bool fe) {
    SegShape sh;
    sh.j = shape_of(v, p, s_max, false, fs, fe, &sh.ring);
    const uint32_t E = std::max<uint32_t>(max_edge(v.C), 1), sb = (uint32_t)sh.j.s_max;
    const size_t row = (size_t)(has_layers(v.C) ? 3 : 1) * sh.j.W * 4;
    uint32_t S = seg ? seg : std::max(E, ceil_sqrt(((uint64_t)sb + 1) * E));
    S = std::min(S, std::max(E, sb + 1));  // a segment longer than the bound is the one segment [0, s']
    sh.S = S;
    sh.nck = sb / S;  // segments 1 .. s' / S
    sh.ck = (size_t)sh.nck * E * row;
    sh.buf = ((size_t)E + S + 1) * row;
    sh.ops = ((size_t)sh.j.n + sh.j.m + 15) & ~size_t(15);
    sh.bytes = sh.ring + sh.ck + sh.buf + sh.ops + kSegPairState;
    return sh;
}

struct EventPool {
    std::vector<hipEvent_t> e;
    bool grow(size_t n) {
        while (e.size() < n) {
            hipEvent_t x = nullptr;
            if (!hip_ok(hipEventCreate(&x), "hipEventCreate")) return false;
            e.push_back(x);
        }
        return true;
    }
    ~EventPool() {
        for (auto& x : e) (void)hipEventDestroy(x);
    }
};

int seg_call(const char* fn, pa_affine_batch* ab, int free_start, int free_end, int32_t s_max, uint32_t seg, int32_t* cost_out, int64_t* start_out,
             int64_t* end_out, std::vector<std::string>* cigars, float* fwd_ms, float* refill_ms, float* walk_ms) {
    const DtView v = dt_view(ab);
    if ((free_start | free_end) & ~1) return fail(PA_E_ARG, "%s: free_start = %d, free_end = %d: each is 0 or 1", fn, free_start, free_end);
    if (s_max < 0 || s_max >= kSMaxLimit) return fail(PA_E_ARG, "%s: s_max = %d outside [0, 2^30)", fn, s_max);
    const uint32_t E = std::max<uint32_t>(max_edge(v.C), 1);
    if (seg != 0 && (seg < E || seg >= (uint32_t)kSMaxLimit))
        return fail(PA_E_ARG, "%s: seg = %u is neither 0 nor in [largest edge, 2^30); the largest edge is %u", fn, seg, E);
    if (!v.trace) return fail(PA_E_ARG, "%s: the batch was created without trace", fn);
    const bool fs = free_start != 0, fe = free_end != 0, ends = fs || fe;
    if (!*v.state) *v.state = new (std::nothrow) DtState;
    DtState* st = *v.state;
    if (!st) return fail(PA_E_NOMEM, "out of memory");
    st->found = st->not_found = st->chunks = st->front_cells = st->extend_chars = st->bytes_max = 0;
    st->seg_chunks = st->seg_rounds = st->seg_jobs = st->seg_refill_cells = st->seg_bytes_max = 0;
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
    std::vector<SegShape> shape(v.np);
    for (size_t p = 0; p < v.np; ++p) {
        shape[p] = seg_shape_of(v, (uint32_t)p, s_max, seg, fs, fe);
        if (shape[p].bytes > budget)
            return fail(PA_E_ARG, "%s: pair %zu: %zu bytes of fronts (s_max %d, %u diagonals, segments of %u) exceed the budget of %zu bytes", fn, p,
                        shape[p].bytes, shape[p].j.s_max, shape[p].j.W - 2, shape[p].S, budget);
    }
    std::vector<uint32_t> order(v.np);  // most expensive first: cost steps x diagonals
    for (size_t p = 0; p < v.np; ++p) order[p] = (uint32_t)p;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return ((uint64_t)shape[x].j.s_max + 1) * shape[x].j.W > ((uint64_t)shape[y].j.s_max + 1) * shape[y].j.W;
    });
    const bool aff = has_layers(v.C);
    const int L = aff ? 3 : 1;
    const CkptFn ckpt = aff ? ckpt_of<true>(fs, fe) : ckpt_of<false>(fs, fe);
    const FillFn fill = aff ? (fs ? dt::affine_dt_fill_kernel<true, true> : dt::affine_dt_fill_kernel<true>)
                            : (fs ? dt::affine_dt_fill_kernel<false, true> : dt::affine_dt_fill_kernel<false>);
    const SegWalkFn walk = aff ? seg_walk_of<true>(fs, fe) : seg_walk_of<false>(fs, fe);
    const size_t cstride = ends ? 2 : 1;
    EventPool ev;
    if (!ev.grow(2) || !st->d_cost.reserve(v.np * cstride * 4) || !st->d_stat.reserve(v.np * sizeof(dt::Stat)) ||
        !hip_ok(hipMemsetAsync(st->d_stat.ptr, 0, v.np * sizeof(dt::Stat), s), "hipMemsetAsync"))
        return PA_E_HIP;
    float fwd_total = 0, refill_total = 0, walk_total = 0;
    std::vector<dt::CkJob> ckjobs;
    std::vector<dt::SegJob> base, jobs;
    std::vector<uint32_t> nseg;
    std::vector<size_t> round_at;
    std::vector<dt::WalkState> state;
    std::vector<dt::Stat> fstat;
    std::vector<uint8_t> ops;
    std::vector<int32_t> cost(v.np * cstride);
    for (size_t c0 = 0; c0 < v.np;) {
        size_t c1 = c0, total = 0;
        while (c1 < v.np && (c1 == c0 || total + shape[order[c1]].bytes <= budget)) total += shape[order[c1]].bytes, ++c1;
        const size_t nj = c1 - c0;
        st->chunks += 1;
        st->seg_chunks += 1;
        st->bytes_max = st->seg_bytes_max = std::max(st->seg_bytes_max, (double)total);
        const size_t fronts_bytes = total - nj * kSegPairState;
        if (!st->d_fronts.reserve(std::max<size_t>(fronts_bytes, 16)) || !st->d_seg_state.reserve(nj * sizeof(dt::WalkState)) ||
            !st->d_seg_stat.reserve(nj * sizeof(dt::Stat)))
            return PA_E_HIP;
        ckjobs.clear();
        base.clear();
        size_t off = 0;
        double wsum = 0;
        for (size_t x = c0; x < c1; ++x) {
            const SegShape& sh = shape[order[x]];
            dt::CkJob K;
            std::memset(&K, 0, sizeof K);
            K.j = sh.j;
            K.j.a = st->d_seq.as<uint8_t>() + v.aoff[sh.j.out];
            K.j.b = st->d_seq.as<uint8_t>() + v.boff[sh.j.out];
            uint8_t* at = st->d_fronts.as<uint8_t>() + off;  // ring | checkpoints | segment buffer | ops
            K.j.fronts = reinterpret_cast<int32_t*>(at);
            K.ck = reinterpret_cast<int32_t*>(at + sh.ring);
            K.S = sh.S, K.nck = sh.nck, K.E = E;
            dt::SegJob G;
            std::memset(&G, 0, sizeof G);
            G.a = K.j.a, G.b = K.j.b;
            G.ck = K.ck;  // (of segment 1; the round's job moves it)
            G.buf = reinterpret_cast<int32_t*>(at + sh.ring + sh.ck);
            G.ops = at + sh.ring + sh.ck + sh.buf;
            G.n = sh.j.n, G.m = sh.j.m, G.W = sh.j.W, G.kmin = sh.j.kmin, G.kmax = sh.j.kmax;
            G.E = E, G.S = sh.S, G.out = sh.j.out, G.slot = (uint32_t)(x - c0);
            off += sh.ring + sh.ck + sh.buf + sh.ops;
            wsum += sh.j.W;
            ckjobs.push_back(K);
            base.push_back(G);
        }
        const int threads = wsum / (double)nj > dt::kWideMean ? dt::kWideBlock : 64;
        if (!st->d_jobs.reserve(nj * sizeof(dt::CkJob)) ||
            !hip_ok(hipMemcpyAsync(st->d_jobs.ptr, ckjobs.data(), nj * sizeof(dt::CkJob), hipMemcpyHostToDevice, s), "H2D") ||
            !hip_ok(hipStreamSynchronize(s), "sync") || !hip_ok(hipEventRecord(ev.e[0], s), "event") ||
            !hip_ok(hipMemsetAsync(st->d_fronts.ptr, dt::kNegByte, std::max<size_t>(fronts_bytes, 16), s), "hipMemsetAsync"))
            return PA_E_HIP;
        hipLaunchKernelGGL(ckpt, dim3((unsigned)nj), dim3(threads), 0, s, st->d_jobs.as<dt::CkJob>(), v.C, st->d_cost.as<int32_t>(), st->d_stat.as<dt::Stat>());
        if (!hip_ok(hipGetLastError(), "affine_dt_ckpt_kernel launch") || !hip_ok(hipEventRecord(ev.e[1], s), "event") ||
            !hip_ok(hipMemcpyAsync(cost.data(), st->d_cost.ptr, cost.size() * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        float f = 0;
        if (!hip_ok(hipEventElapsedTime(&f, ev.e[0], ev.e[1]), "hipEventElapsedTime")) return PA_E_HIP;
        fwd_total += f;
        // the rounds follow from the costs: pair x stands in segment nseg[x] - 1 - r in round r
        nseg.assign(nj, 0);
        state.assign(nj, dt::WalkState{0, 0, 0, 0, 0, 0});
        uint32_t rounds = 0;
        size_t njobs = 0;
        for (size_t x = 0; x < nj; ++x) {
            const uint32_t p = base[x].out;
            const int32_t c = cost[cstride * p];
            if (c < 0) continue;
            nseg[x] = (uint32_t)c / base[x].S + 1;
            rounds = std::max(rounds, nseg[x]);
            njobs += nseg[x];
            const int32_t i = ends ? cost[2 * (size_t)p + 1] : (int32_t)base[x].n;
            state[x] = dt::WalkState{c, 0, i, i - (int32_t)base[x].m, 0, 0};
        }
        st->seg_rounds += rounds;
        st->seg_jobs += (double)njobs;
        if (rounds) {
            jobs.clear();
            jobs.reserve(njobs);
            round_at.assign(rounds + 1, 0);
            for (uint32_t r = 0; r < rounds; ++r) {
                for (size_t x = 0; x < nj; ++x) {
                    if (nseg[x] <= r) continue;
                    dt::SegJob G = base[x];
                    const uint32_t c = nseg[x] - 1 - r;
                    G.s0 = (int32_t)(c * G.S);
                    G.s1 = (int32_t)std::min<uint64_t>((uint64_t)G.s0 + G.S - 1, (uint64_t)cost[cstride * G.out]);
                    G.ck = c ? G.ck + (size_t)(c - 1) * E * L * G.W : nullptr;
                    jobs.push_back(G);
                }
                round_at[r + 1] = jobs.size();
            }
            if (!ev.grow(2 * (size_t)rounds + 1) || !st->d_seg_jobs.reserve(jobs.size() * sizeof(dt::SegJob)) ||
                !hip_ok(hipMemcpyAsync(st->d_seg_jobs.ptr, jobs.data(), jobs.size() * sizeof(dt::SegJob), hipMemcpyHostToDevice, s), "H2D") ||
                !hip_ok(hipMemcpyAsync(st->d_seg_state.ptr, state.data(), nj * sizeof(dt::WalkState), hipMemcpyHostToDevice, s), "H2D") ||
                !hip_ok(hipMemsetAsync(st->d_seg_stat.ptr, 0, nj * sizeof(dt::Stat), s), "hipMemsetAsync") ||
                !hip_ok(hipStreamSynchronize(s), "sync") ||  // (jobs and state are pageable memory; state is read back into)
                !hip_ok(hipEventRecord(ev.e[0], s), "event"))
                return PA_E_HIP;
            for (uint32_t r = 0; r < rounds; ++r) {
                const dt::SegJob* dj = st->d_seg_jobs.as<dt::SegJob>() + round_at[r];
                const size_t cnt = round_at[r + 1] - round_at[r];
                double w = 0;  // the wide-block rule, over the jobs of this launch
                for (size_t x = round_at[r]; x < round_at[r + 1]; ++x) w += jobs[x].W;
                const int fill_threads = w / (double)cnt > dt::kWideMean ? dt::kWideBlock : 64;
                hipLaunchKernelGGL(fill, dim3((unsigned)cnt), dim3(fill_threads), 0, s, dj, v.C, st->d_seg_stat.as<dt::Stat>());
                if (!hip_ok(hipGetLastError(), "affine_dt_fill_kernel launch") || !hip_ok(hipEventRecord(ev.e[2 * r + 1], s), "event")) return PA_E_HIP;
                hipLaunchKernelGGL(walk, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, s, dj, (int)cnt, v.C, st->d_seg_state.as<dt::WalkState>());
                if (!hip_ok(hipGetLastError(), "affine_dt_seg_walk_kernel launch") || !hip_ok(hipEventRecord(ev.e[2 * r + 2], s), "event")) return PA_E_HIP;
            }
            fstat.resize(nj);
            if (!hip_ok(hipMemcpyAsync(state.data(), st->d_seg_state.ptr, nj * sizeof(dt::WalkState), hipMemcpyDeviceToHost, s), "D2H") ||
                !hip_ok(hipMemcpyAsync(fstat.data(), st->d_seg_stat.ptr, nj * sizeof(dt::Stat), hipMemcpyDeviceToHost, s), "D2H") ||
                !hip_ok(hipStreamSynchronize(s), "sync"))
                return PA_E_HIP;
            for (uint32_t r = 0; r < rounds; ++r) {
                float a = 0, b = 0;
                if (!hip_ok(hipEventElapsedTime(&a, ev.e[2 * r], ev.e[2 * r + 1]), "hipEventElapsedTime") ||
                    !hip_ok(hipEventElapsedTime(&b, ev.e[2 * r + 1], ev.e[2 * r + 2]), "hipEventElapsedTime"))
                    return PA_E_HIP;
                refill_total += a;
                walk_total += b;
            }
            std::vector<size_t> at(nj + 1, 0);  // every found pair's ops lie behind its segment buffer: one copy per pair
            for (size_t x = 0; x < nj; ++x) {
                if (state[x].status != 0)
                    return fail(PA_E_INTERNAL, "%s: pair %u: %s", fn, base[x].out, state[x].status == 1 ? "a front holds no parent" : "path longer than its buffer");
                at[x + 1] = at[x] + (nseg[x] ? (size_t)state[x].nops : 0);
                st->seg_refill_cells += (double)fstat[x].front_cells;
            }
            ops.resize(at.back());
            for (size_t x = 0; x < nj; ++x)
                if (at[x + 1] > at[x] && !hip_ok(hipMemcpyAsync(ops.data() + at[x], base[x].ops, at[x + 1] - at[x], hipMemcpyDeviceToHost, s), "D2H"))
                    return PA_E_HIP;
            if (!hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
            for (size_t x = 0; x < nj; ++x) {
                if (!nseg[x]) continue;
                (*cigars)[base[x].out] = cigar_of(ops.data() + at[x], (int32_t)(at[x + 1] - at[x]));
                start_out[base[x].out] = (int64_t)std::count_if(ops.data() + at[x], ops.data() + at[x + 1], [](uint8_t op) { return op != 'I'; });
            }
        }
        c0 = c1;
    }
    std::vector<dt::Stat> stat(v.np);
    if (!hip_ok(hipMemcpyAsync(stat.data(), st->d_stat.ptr, v.np * sizeof(dt::Stat), hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    for (size_t p = 0; p < v.np; ++p) {
        const int32_t c = cost[cstride * p];
        const int64_t end = c < 0 ? -1 : ends ? cost[2 * p + 1] : (int64_t)v.n[p];
        if (cost_out) cost_out[p] = c;
        if (end_out) end_out[p] = end;
        start_out[p] = end < 0 ? -1 : end - start_out[p];  // (the path's bytes of a were counted there)
        (c >= 0 ? st->found : st->not_found) += 1;
        st->front_cells += (double)stat[p].front_cells;
        st->extend_chars += (double)stat[p].extend_chars;
    }
    if (fwd_ms) *fwd_ms = fwd_total;
    if (refill_ms) *refill_ms = refill_total;
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

extern "C" int pa_affine_batch_align_dt_seg(pa_affine_batch* ab, int free_start, int free_end, int32_t s_max, uint32_t seg, int32_t* cost_out,
                                            int64_t* start_out, int64_t* end_out, char** cigar_out, float* forward_ms, float* refill_ms, float* walk_ms) {
    if (forward_ms) *forward_ms = 0;
    if (refill_ms) *refill_ms = 0;
    if (walk_ms) *walk_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_align_dt_seg: NULL batch");
    const size_t np = dt_view(ab).np;
    if (cigar_out)
        for (size_t p = 0; p < np; ++p) cigar_out[p] = nullptr;
    std::vector<std::string> cigars(np);
    std::vector<int64_t> start(np);  // (seg_call counts the path's bytes of a here before it knows the ends)
    if (const int rc = seg_call("pa_affine_batch_align_dt_seg", ab, free_start, free_end, s_max, seg, cost_out, start.data(), end_out, &cigars, forward_ms,
                                refill_ms, walk_ms))
        return rc;
    if (start_out) std::copy(start.begin(), start.end(), start_out);
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" void pa_affine_batch_dt_seg_info(const pa_affine_batch* ab, double* chunks, double* rounds, double* seg_jobs, double* refill_cells,
                                            double* bytes_max) {
    const DtState* st = ab ? *dt_view(const_cast<pa_affine_batch*>(ab)).state : nullptr;
    if (chunks) *chunks = st ? st->seg_chunks : 0;
    if (rounds) *rounds = st ? st->seg_rounds : 0;
    if (seg_jobs) *seg_jobs = st ? st->seg_jobs : 0;
    if (refill_cells) *refill_cells = st ? st->seg_refill_cells : 0;
    if (bytes_max) *bytes_max = st ? st->seg_bytes_max : 0;
}
