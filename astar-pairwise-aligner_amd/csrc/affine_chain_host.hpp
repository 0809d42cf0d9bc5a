// affine_chain_host.hpp -- the host side of the chained route, written once for both gap-affine batches (two layers: affine_unit.hip
// and affine_chain_kernel; four layers: affine4_unit.hip, affine4_tiled_unit.hip and affine4_chain_kernel).  The plan is
// affine_chain_plan.hpp's, in boundary values of T::kLayout.bnd_bytes bytes; here it becomes jobs, launches and the error check.
//
// As in affine_host.hpp no kernel is named here.  A unit's traits T add, to what that header lists:
//   ChainJob                             the kernel's job record {pair, strip, bnd_in, bnd_out}
//   Batch::chain                         a ChainState
//   launch_chain_run(ab, d_jobs, njobs, d_pairs, ticket_err, s)              the cost-only chained kernel over one chunk's jobs
//   launch_chain_ckpt(ab, d_jobs, njobs, d_pairs, tile_cols, ticket_err, s)  the checkpointing one
//   launch_ckpt(ab, d_waves, nwaves, d_pairs, s)                             the unchained checkpoint kernel over nwaves device waves
// and, as everywhere, only what the templates a unit instantiates use: run_chained() needs launch<false> and launch_chain_run,
// ckpt_pass() needs launch_ckpt and launch_chain_ckpt.
#pragma once
#include "affine_host.hpp"
#include "affine_chain_plan.hpp"

namespace pa {
namespace affine_host {

// The chained route's part of a batch (set_chain): the packed pairs keep a plan of their own, the others are listed in planner order.
template <class PlanT>
struct ChainState {
    bool on = false, built = false;
    std::vector<uint32_t> ids;  // pairs with |b| > 1024, in planner order
    PlanT packed;               // the plan of the rest
    DeviceBuf d_pairs;          // Pair of every id
    DeviceBuf d_jobs, d_bnd, d_ticket_err;
    double pairs = 0, jobs = 0, chunks = 0, bnd_bytes_max = 0;  // the last chained pass
};

// The counters are those of the last chained pass: a run() or an align_tiled() with chaining on starts them again.
template <class BatchT>
void chain_begin(BatchT& ab) {
    if (ab.chain.on) ab.chain.pairs = ab.chain.jobs = ab.chain.chunks = ab.chain.bnd_bytes_max = 0;
}

// The device jobs of a chain plan, chunk after chunk, every chunk's rows at `rows`.  Pair p of the plan is pair at[p] of the kernel's Pair
// array (p itself without `at`).
template <class T>
std::vector<typename T::ChainJob> chain_jobs_of(const affine_chain::Plan& cp, const std::vector<affine_chain::Shape>& shapes, void* rows,
                                                const std::vector<uint32_t>* at = nullptr) {
    using ChainJob = typename T::ChainJob;
    constexpr size_t vb = T::kLayout.bnd_bytes;
    std::vector<ChainJob> jobs;
    jobs.reserve(cp.jobs.size());
    for (const affine_chain::Job& q : cp.jobs) {
        const size_t S = affine_chain::strips_of(shapes[q.pair].m), w = affine_chain::row_words(shapes[q.pair].n) * vb;  // w: bytes of a row
        uint8_t* row0 = static_cast<uint8_t*>(rows) + cp.row_off[q.pair] * vb;
        ChainJob J;
        J.pair = at ? (*at)[q.pair] : q.pair;
        J.strip = q.strip;
        J.bnd_in = q.strip ? reinterpret_cast<decltype(J.bnd_in)>(row0 + (size_t)(q.strip - 1) * w) : nullptr;
        J.bnd_out = q.strip + 1 < S ? reinterpret_cast<decltype(J.bnd_out)>(row0 + (size_t)q.strip * w) : nullptr;
        jobs.push_back(J);
    }
    return jobs;
}

// One chained pass, a launch per chunk of the plan: ticket and error word cleared and the chunk's rows (at `rows`) set to all-ones on the
// stream, launch_kernel(the chunk's jobs, their number, ticket_err) over the jobs at d_jobs (chain_jobs_of), and the copy of its error
// word to errs, for chain_check to read once the stream is synchronised.  Counts the pass in chain.*.
template <class T, class Launch>
bool launch_chain(typename T::Batch& ab, const affine_chain::Plan& cp, const typename T::ChainJob* d_jobs, void* rows, std::vector<uint32_t>& errs,
                  hipStream_t s, Launch launch_kernel) {
    constexpr size_t vb = T::kLayout.bnd_bytes;
    uint32_t* te = ab.chain.d_ticket_err.template as<uint32_t>();
    errs.assign(cp.chunks.size(), 0);
    for (size_t k = 0; k < cp.chunks.size(); ++k) {
        const affine_chain::Chunk& c = cp.chunks[k];
        if (!hip_ok(hipMemsetAsync(te, 0, 8, s), "hipMemsetAsync") || (c.words && !hip_ok(hipMemsetAsync(rows, 0xFF, c.words * vb, s), "hipMemsetAsync")))
            return false;
        if (!launch_kernel(d_jobs + c.first_job, (int)c.njobs, te) || !hip_ok(hipMemcpyAsync(&errs[k], te + 1, 4, hipMemcpyDeviceToHost, s), "D2H"))
            return false;
    }
    ab.chain.pairs += (double)cp.row_off.size();
    ab.chain.jobs += (double)cp.jobs.size();
    ab.chain.chunks += (double)cp.chunks.size();
    ab.chain.bnd_bytes_max = std::max(ab.chain.bnd_bytes_max, (double)(cp.words_max * vb));
    return true;
}

template <class T>
int chain_check(const char* fn, const std::vector<uint32_t>& errs) {
    uint32_t err = 0;
    for (const uint32_t e : errs)
        if (e) err = e;
    if (!err) return 0;
    return fail(PA_E_INTERNAL, "%s_%s: chained route: a strip never received its boundary row (device spin timeout, err=%u); no result of this call is valid",
                T::kName, fn, err);
}

// What set_chain(1) needs once: the chained pairs, their Pair array and the plan of the packed rest.
template <class T>
int chain_build(typename T::Batch& ab, hipStream_t s) {
    using Pair = typename T::Pair;
    if (ab.chain.built) return 0;
    std::vector<uint32_t> rest;
    ab.chain.ids.clear();  // (an earlier attempt may have failed half-way)
    for (const uint32_t p : ab.order) (ab.m[p] > affine_chain::kStripRows ? ab.chain.ids : rest).push_back(p);
    std::vector<Pair> pairs;
    for (const uint32_t p : ab.chain.ids) pairs.push_back(make_pair<T>(ab, p, (uint32_t)affine_plan::rows_of(T::kLayout, ab.m[p])));
    if (!upload(ab.chain.d_pairs, pairs.data(), pairs.size() * sizeof(Pair), s) || !ab.chain.d_ticket_err.alloc(16)) return PA_E_HIP;
    if (!ab.chain.ids.empty())  // (without chained pairs run() keeps the batch's own plan)
        if (const int rc = make_plan<T>(ab, rest, ab.chain.packed, Keep::kNone, nullptr, s)) return rc;
    if (!hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
    ab.chain.built = true;
    return 0;
}

// *_batch_set_chain.
template <class T>
int set_chain(typename T::Batch* ab, int on) {
    static_assert(size_t(64) * T::kLayout.rows == affine_chain::kStripRows, "affine_chain_plan.hpp plans the strips of this layout");
    if (!ab) return fail(PA_E_ARG, "%s_set_chain: NULL batch", T::kName);
    if (on != 0 && on != 1) return fail(PA_E_ARG, "%s_set_chain: on = %d is neither 0 nor 1", T::kName, on);
    if (on)
        if (const int rc = chain_build<T>(*ab, 0)) return rc;
    ab->chain.on = on != 0;
    return 0;
}

// *_batch_chain_info.
template <class BatchT>
void chain_info(const BatchT* ab, double* on, double* chain_pairs, double* chain_jobs, double* chunks, double* bnd_bytes_max) {
    if (on) *on = ab && ab->chain.on ? 1 : 0;
    if (chain_pairs) *chain_pairs = ab ? ab->chain.pairs : 0;
    if (chain_jobs) *chain_jobs = ab ? ab->chain.jobs : 0;
    if (chunks) *chunks = ab ? ab->chain.chunks : 0;
    if (bnd_bytes_max) *bnd_bytes_max = ab ? ab->chain.bnd_bytes_max : 0;
}

// run() with chaining on and pairs to chain: the packed pairs' launch, then the chained pairs in chunks whose boundary rows fit the budget.
template <class T>
int run_chained(typename T::Batch& ab, Events& ev, hipStream_t s) {
    using ChainJob = typename T::ChainJob;
    using Pair = typename T::Pair;
    constexpr size_t vb = T::kLayout.bnd_bytes;
    std::vector<affine_chain::Shape> shapes;
    for (const uint32_t p : ab.chain.ids) shapes.push_back(affine_chain::Shape{ab.n[p], ab.m[p]});
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    const affine_chain::Plan cp = affine_chain::plan(shapes, budget, vb);
    if (cp.refused >= 0)
        return fail(PA_E_ARG, "%s_run: pair %u: %zu bytes of boundary rows of the chained route exceed the budget of %zu bytes", T::kName,
                    ab.chain.ids[(size_t)cp.refused], affine_chain::pair_bytes(shapes[(size_t)cp.refused], vb), budget);
    if (!ab.chain.d_bnd.reserve(std::max<size_t>(cp.words_max * vb, 16))) return PA_E_HIP;
    const std::vector<ChainJob> jobs = chain_jobs_of<T>(cp, shapes, ab.chain.d_bnd.ptr);
    std::vector<uint32_t> errs;
    const Pair* d_pairs = ab.chain.d_pairs.template as<Pair>();
    if (!ab.chain.d_jobs.reserve(jobs.size() * sizeof(ChainJob)) ||
        !hip_ok(hipMemcpyAsync(ab.chain.d_jobs.ptr, jobs.data(), jobs.size() * sizeof(ChainJob), hipMemcpyHostToDevice, s), "H2D") ||
        !hip_ok(hipStreamSynchronize(s), "sync") ||  // (jobs is pageable memory of this call)
        !hip_ok(hipEventRecord(ev.e[0], s), "event") || !T::template launch<false>(ab, ab.chain.packed, s) ||
        !launch_chain<T>(ab, cp, ab.chain.d_jobs.template as<ChainJob>(), ab.chain.d_bnd.ptr, errs, s,
                         [&](const ChainJob* j, int nj, uint32_t* te) { return T::launch_chain_run(ab, j, nj, d_pairs, te, s); }) ||
        !hip_ok(hipEventRecord(ev.e[1], s), "event") || !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    return chain_check<T>("run", errs);
}

// The checkpoint pass of a chunk of align_tiled, timed, the stream synchronised: the chunk's plan with the unchained checkpoint kernel
// or, with chaining on, its one-strip waves with that kernel and the strip pairs chained, into the rows make_plan has placed.  Under a
// free end the walks are then seeded with the ends it found (seed_walks).
template <class T>
int ckpt_pass(typename T::Batch& ab, TiledChunk<T>& ch, uint32_t C, hipStream_t s, float* ms) {
    using ChainJob = typename T::ChainJob;
    using Pair = typename T::Pair;
    using Wave = typename T::Wave;
    constexpr size_t vb = T::kLayout.bnd_bytes;
    auto& P = ch.plan;
    const size_t np = P.pairs.size();
    Events ev;
    if (!ev.make()) return PA_E_HIP;
    DeviceBuf d_pwaves, d_cjobs;  // chained: the plan's one-strip waves, and the chain jobs of the others
    const Wave* d_waves = P.d_waves.template as<Wave>();
    size_t nwaves = P.waves.size();
    affine_chain::Plan cp;
    if (ab.chain.on) {  // the strip pairs leave the plan's launch for the chained one; their rows stay where make_plan put them
        std::vector<Wave> one;
        std::vector<affine_chain::Shape> shapes;
        std::vector<uint32_t> at;  // index into P.pairs
        for (const Wave& W : P.waves)
            if (W.strips == 1) one.push_back(W);
        for (size_t k = 0; k < np; ++k)  // (P.pairs keeps the order of ids; the waves are sorted by cost)
            if (P.pairs[k].m > affine_chain::kStripRows) {
                shapes.push_back(affine_chain::Shape{P.pairs[k].n, P.pairs[k].m});
                at.push_back((uint32_t)k);
            }
        cp = affine_chain::plan(shapes, SIZE_MAX, vb);  // (this chunk was cut by tiled_bytes_of, which counts the rows)
        for (size_t x = 0; x < shapes.size(); ++x)
            if (cp.chunks.size() != 1 || ch.rowck[at[x]] != P.d_bnd.template as<uint8_t>() + cp.row_off[x] * vb || cp.words_max != P.at.bnd_vals)
                return fail(PA_E_INTERNAL, "%s_align_tiled: chained route: the planner and the checkpoint plan disagree on pair %u's rows", T::kName,
                            P.pairs[at[x]].out);
        const std::vector<ChainJob> cjobs = chain_jobs_of<T>(cp, shapes, P.d_bnd.ptr, &at);
        if (!upload(d_pwaves, one.data(), one.size() * sizeof(Wave), s) || !upload(d_cjobs, cjobs.data(), cjobs.size() * sizeof(ChainJob), s) ||
            !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        d_waves = d_pwaves.template as<Wave>();
        nwaves = one.size();
    }
    std::vector<uint32_t> errs;
    const Pair* d_pairs = P.d_pairs.template as<Pair>();
    if (!hip_ok(hipEventRecord(ev.e[0], s), "event") || !T::launch_ckpt(ab, d_waves, nwaves, d_pairs, s) ||
        !launch_chain<T>(ab, cp, d_cjobs.template as<ChainJob>(), P.d_bnd.ptr, errs, s,
                         [&](const ChainJob* j, int nj, uint32_t* te) { return T::launch_chain_ckpt(ab, j, nj, d_pairs, C, te, s); }) ||
        !hip_ok(hipEventRecord(ev.e[1], s), "event") || !hip_ok(hipStreamSynchronize(s), "sync") ||
        !hip_ok(hipEventElapsedTime(ms, ev.e[0], ev.e[1]), "hipEventElapsedTime"))
        return PA_E_HIP;
    if (const int rc = chain_check<T>("align_tiled", errs)) return rc;
    return seed_walks<T>(ab, ch, s);  // a free end: every walk starts at the end this pass found
}

}  // namespace affine_host
}  // namespace pa
