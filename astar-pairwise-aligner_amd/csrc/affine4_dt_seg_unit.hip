// affine4_dt_seg_unit.hip -- the segmented traceback of the double-affine diagonal-transition route: pa_affine4_batch_align_dt_seg and
// _dt_seg_info (include/pa_affine4_dt_seg_hip.h).  The results of pa_affine4_batch_align_dt_ends in device memory that grows with the
// square root of the bound (affine4_dt_seg_plan.hpp has the argument, the geometry and the bytes; affine4_dt_seg_kernel.hpp the three
// kernels): a checkpointing pass over the five rings, the costs read back once, then per round one launch that re-fills a segment of
// fronts for every unfinished pair and one that walks it, with no host round trip between the rounds; the states and ops are read
// back once after the last round.
//
// The driver restates affine_dt_unit.hip's seg_call over this batch's plan, job records and kernels; sharing it between the two
// batches is left to a change that may touch that unit.
#include "pa_hip_internal.hpp"
#include "affine4_dt_seg_kernel.hpp"
#include "affine4_dt_seg_plan.hpp"
#include "affine4_dt_host.hpp"
#include "affine4_dt_view.hpp"
#include "../../include/pa_affine4_dt_seg_hip.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace pa;
using namespace pa::affine4;

namespace {

static_assert(sizeof(dt::WalkState) + sizeof(dt::Stat) == dt::kSegPairState, "the per-pair state of affine4_dt_seg_plan.hpp");

using CkptFn = void (*)(const dt::CkJob*, dt::Costs, dt::SegRows, int32_t*, dt::Stat*);
using FillFn = void (*)(const dt::SegJob*, dt::Costs, dt::SegRows, dt::Stat*);
using SegWalkFn = void (*)(const dt::SegJob*, int, dt::Costs, dt::SegRows, dt::WalkState*);
CkptFn ckpt_of(bool fs, bool fe) {
    return fs ? (fe ? dt::affine4_dt_ckpt_kernel<true, true> : dt::affine4_dt_ckpt_kernel<true, false>)
              : (fe ? dt::affine4_dt_ckpt_kernel<false, true> : dt::affine4_dt_ckpt_kernel<>);
}
SegWalkFn seg_walk_of(bool fs, bool fe) {
    return fs ? (fe ? dt::affine4_dt_seg_walk_kernel<true, true> : dt::affine4_dt_seg_walk_kernel<true, false>)
              : (fe ? dt::affine4_dt_seg_walk_kernel<false, true> : dt::affine4_dt_seg_walk_kernel<>);
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

int seg_call(const char* fn, pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, uint32_t seg, int32_t* cost_out, int64_t* start_out,
             int64_t* end_out, std::vector<std::string>* cigars, float* fwd_ms, float* refill_ms, float* walk_ms) {
    const DtView v = dt_view(ab);
    if ((free_start | free_end) & ~1) return fail(PA_E_ARG, "%s: free_start = %d, free_end = %d: each is 0 or 1", fn, free_start, free_end);
    if (s_max < 0 || s_max >= kSMaxLimit) return fail(PA_E_ARG, "%s: s_max = %d outside [0, 2^30)", fn, s_max);
    const dt::SegRows G = dt::seg_rows(v.C);
    if (seg != 0 && (seg < G.Ew || seg >= (uint32_t)kSMaxLimit))
        return fail(PA_E_ARG, "%s: seg = %u is neither 0 nor in [Ew, 2^30); Ew, the largest of the edges and extends, is %u", fn, seg, G.Ew);
    if (!v.trace) return fail(PA_E_ARG, "%s: the batch was created without trace", fn);
    const bool fs = free_start != 0, fe = free_end != 0, ends = fs || fe;
    if (!*v.state) *v.state = new (std::nothrow) DtState;
    DtState* st = *v.state;
    if (!st) return fail(PA_E_NOMEM, "out of memory");
    st->found = st->not_found = st->chunks = st->front_cells = st->extend_chars = st->bytes_max = 0;
    st->seg_chunks = st->seg_rounds = st->seg_jobs = st->seg_refill_cells = st->seg_bytes_max = 0;
    if (v.np == 0) return 0;
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    const dt::SegPlan P = dt::seg_plan(v.n, v.m, v.np, v.C, s_max, seg, fs, fe, budget);
    if (P.refused >= 0) {
        const dt::SegShape& sh = P.shape[(size_t)P.refused];
        return fail(PA_E_ARG, "%s: pair %lld: %zu bytes of fronts (s_max %d, %u diagonals, segments of %u) exceed the budget of %zu bytes", fn, P.refused,
                    sh.bytes, sh.ring.s_max, sh.ring.W - 2, sh.S, budget);
    }
    hipStream_t s = 0;
    if (!st->seq_ready) {
        if (!st->d_seq.alloc(v.seq_bytes + dt::kSeqPad) ||
            (v.seq_bytes && !hip_ok(hipMemcpyAsync(st->d_seq.ptr, v.d_seq, v.seq_bytes, hipMemcpyDeviceToDevice, s), "D2D")) ||
            !hip_ok(hipMemsetAsync(st->d_seq.as<uint8_t>() + v.seq_bytes, 0, dt::kSeqPad, s), "hipMemsetAsync"))
            return PA_E_HIP;
        st->seq_ready = true;
    }
    const CkptFn ckpt = ckpt_of(fs, fe);
    const FillFn fill = fs ? dt::affine4_dt_fill_kernel<true> : dt::affine4_dt_fill_kernel<>;
    const SegWalkFn walk = seg_walk_of(fs, fe);
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
    for (const dt::Chunk& ch : P.chunks) {
        const size_t nj = ch.count;
        st->chunks += 1;
        st->seg_chunks += 1;
        st->bytes_max = st->seg_bytes_max = std::max(st->seg_bytes_max, (double)ch.bytes);
        const size_t fronts_bytes = ch.bytes - nj * dt::kSegPairState;
        if (!st->d_fronts.reserve(std::max<size_t>(fronts_bytes, 16)) || !st->d_seg_state.reserve(nj * sizeof(dt::WalkState)) ||
            !st->d_seg_stat.reserve(nj * sizeof(dt::Stat)))
            return PA_E_HIP;
        ckjobs.clear();
        base.clear();
        for (size_t x = ch.first; x < ch.first + ch.count; ++x) {
            const uint32_t p = P.order[x];
            const dt::SegShape& sh = P.shape[p];
            dt::CkJob K;
            std::memset(&K, 0, sizeof K);
            dt::Job& J = K.j;
            J.a = st->d_seq.as<uint8_t>() + v.aoff[p];
            J.b = st->d_seq.as<uint8_t>() + v.boff[p];
            uint8_t* at = st->d_fronts.as<uint8_t>() + P.off[p];  // ring | checkpoints | segment buffer | ops
            J.fronts = reinterpret_cast<int32_t*>(at);
            J.n = sh.ring.n, J.m = sh.ring.m, J.s_max = sh.ring.s_max, J.W = sh.ring.W, J.kmin = sh.ring.kmin, J.kmax = sh.ring.kmax, J.out = p;
            for (int t = 0; t < 5; ++t) J.depth[t] = sh.ring.depth[t];
            K.ck = reinterpret_cast<int32_t*>(at + sh.ring_bytes);
            K.S = sh.S, K.nck = sh.nseg - 1;
            dt::SegJob Q;
            std::memset(&Q, 0, sizeof Q);
            Q.a = J.a, Q.b = J.b;
            Q.ck = K.ck;  // (of segment 1; the round's job moves it)
            Q.buf = reinterpret_cast<int32_t*>(at + sh.ring_bytes + sh.ck_bytes);
            Q.ops = at + sh.ring_bytes + sh.ck_bytes + sh.buf_bytes;
            Q.n = J.n, Q.m = J.m, Q.W = J.W, Q.kmin = J.kmin, Q.kmax = J.kmax;
            Q.S = sh.S, Q.out = p, Q.slot = (uint32_t)(x - ch.first);
            ckjobs.push_back(K);
            base.push_back(Q);
        }
        const int threads = ch.wide ? dt::kWideBlock : 64;
        if (!st->d_jobs.reserve(nj * sizeof(dt::CkJob)) ||
            !hip_ok(hipMemcpyAsync(st->d_jobs.ptr, ckjobs.data(), nj * sizeof(dt::CkJob), hipMemcpyHostToDevice, s), "H2D") ||
            !hip_ok(hipStreamSynchronize(s), "sync") || !hip_ok(hipEventRecord(ev.e[0], s), "event") ||
            !hip_ok(hipMemsetAsync(st->d_fronts.ptr, dt::kNegByte, std::max<size_t>(fronts_bytes, 16), s), "hipMemsetAsync"))
            return PA_E_HIP;
        hipLaunchKernelGGL(ckpt, dim3((unsigned)nj), dim3(threads), 0, s, st->d_jobs.as<dt::CkJob>(), v.C, G, st->d_cost.as<int32_t>(), st->d_stat.as<dt::Stat>());
        if (!hip_ok(hipGetLastError(), "affine4_dt_ckpt_kernel launch") || !hip_ok(hipEventRecord(ev.e[1], s), "event") ||
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
                    dt::SegJob Q = base[x];
                    const uint32_t c = nseg[x] - 1 - r;
                    Q.s0 = (int32_t)(c * Q.S);
                    Q.s1 = (int32_t)std::min<uint64_t>((uint64_t)Q.s0 + Q.S - 1, (uint64_t)cost[cstride * Q.out]);
                    Q.ck = c ? Q.ck + (size_t)(c - 1) * G.H * Q.W : nullptr;
                    jobs.push_back(Q);
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
                hipLaunchKernelGGL(fill, dim3((unsigned)cnt), dim3(fill_threads), 0, s, dj, v.C, G, st->d_seg_stat.as<dt::Stat>());
                if (!hip_ok(hipGetLastError(), "affine4_dt_fill_kernel launch") || !hip_ok(hipEventRecord(ev.e[2 * r + 1], s), "event")) return PA_E_HIP;
                hipLaunchKernelGGL(walk, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, s, dj, (int)cnt, v.C, G, st->d_seg_state.as<dt::WalkState>());
                if (!hip_ok(hipGetLastError(), "affine4_dt_seg_walk_kernel launch") || !hip_ok(hipEventRecord(ev.e[2 * r + 2], s), "event")) return PA_E_HIP;
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
                // the bytes of a the path consumes (every op but an insertion's): start = end - these
                start_out[base[x].out] = (int64_t)std::count_if(ops.data() + at[x], ops.data() + at[x + 1],
                                                                [](uint8_t op) { return op != 'I' && op != 'i' && op != 'j'; });
            }
        }
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

extern "C" int pa_affine4_batch_align_dt_seg(pa_affine4_batch* ab, int free_start, int free_end, int32_t s_max, uint32_t seg, int32_t* cost_out,
                                             int64_t* start_out, int64_t* end_out, char** cigar_out, float* forward_ms, float* refill_ms, float* walk_ms) {
    if (forward_ms) *forward_ms = 0;
    if (refill_ms) *refill_ms = 0;
    if (walk_ms) *walk_ms = 0;
    if (!ab) return fail(PA_E_ARG, "pa_affine4_batch_align_dt_seg: NULL batch");
    const size_t np = dt_view(ab).np;
    if (cigar_out)
        for (size_t p = 0; p < np; ++p) cigar_out[p] = nullptr;
    std::vector<std::string> cigars(np);
    std::vector<int64_t> start(np);  // (seg_call counts the path's bytes of a here before it knows the ends)
    if (const int rc = seg_call("pa_affine4_batch_align_dt_seg", ab, free_start, free_end, s_max, seg, cost_out, start.data(), end_out, &cigars, forward_ms,
                                refill_ms, walk_ms))
        return rc;
    if (start_out) std::copy(start.begin(), start.end(), start_out);
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" void pa_affine4_batch_dt_seg_info(const pa_affine4_batch* ab, double* chunks, double* rounds, double* seg_jobs, double* refill_cells,
                                             double* bytes_max) {
    const DtState* st = ab ? *dt_view(const_cast<pa_affine4_batch*>(ab)).state : nullptr;
    if (chunks) *chunks = st ? st->seg_chunks : 0;
    if (rounds) *rounds = st ? st->seg_rounds : 0;
    if (seg_jobs) *seg_jobs = st ? st->seg_jobs : 0;
    if (refill_cells) *refill_cells = st ? st->seg_refill_cells : 0;
    if (bytes_max) *bytes_max = st ? st->seg_bytes_max : 0;
}
