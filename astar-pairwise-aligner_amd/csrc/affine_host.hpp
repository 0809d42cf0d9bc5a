// affine_host.hpp -- the host side that both gap-affine batches share (two layers: affine_unit.hip; four layers: affine4_unit.hip and
// affine4_tiled_unit.hip): the batch's common part, the tail of create, make_plan, and the drivers of align() and align_tiled().  The
// arithmetic is affine_plan.hpp's; here its offsets become the kernels' records and its chunks become launches.
//
// No kernel is named here: the kernels are non-template __global__ functions defined in headers and must stay in one unit each.  A unit
// includes its kernel header, then this one, and instantiates the templates with a traits struct T of its own:
//   Batch, Pair, Wave, Walk, WalkOut, WalkState, TileJob, TileWave   the records
//   kLayout                              affine_plan.hpp's description of the batch type
//   kName                                the C prefix that begins every error text ("pa_affine_batch")
//   kMaxLayer, kVisitSlack               the highest layer of a walk state; what the visit guard allows beyond tile_visits_max
//   launch<FILL>(ab, P, s)               the cost / fill kernel over a plan
//   walk_extra(ab, Q, w), launch_walk(ab, d_walks, nw, d_outs, s), walk_start(o)   the walk over a chunk's codes
//   begin_tiled(ab)                      what else a batch resets when an align_tiled() call starts its work
//   ckpt_pass(ab, ch, C, s, ms)          the checkpoint pass over ch.plan, timed, the stream synchronised
//   launch_tile_fill(ab, d_waves, nw, d_jobs, s), launch_tile_walk(ab, d_jobs, nj, s)
//   walk_done(ab, S)                     whether a walk state needs no further tile
//   cigar_of(ops, nops)                  the CIGAR text of a walk's ops
//   finish(ab, cost_out, s, starts)      the costs to the caller, and whatever else the batch keeps of a call
// and for ends-free mode (set_free_ends, batch_ends, last_row, costs_out, seed_walks: near the end of this header) ends_flags,
// set_ends_flags and launch_rows.
// A unit's traits need only what the templates it instantiates use.
#pragma once
#include "pa_hip_internal.hpp"
#include "affine_plan.hpp"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace pa {
namespace affine_host {

using affine_plan::Keep;

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

// One launch's worth of waves over a subset of the pairs.
template <class PairT, class WaveT>
struct Plan {
    using Wave = WaveT;
    std::vector<WaveT> waves;
    std::vector<PairT> pairs;
    affine_plan::Waves at;  // what the records were made from: pairs[k] is at.pairs[k]
    DeviceBuf d_waves, d_pairs, d_bnd;
};

// What every batch type keeps.
template <class PairT, class WaveT>
struct Batch {
    size_t np = 0;
    bool trace = false;
    std::vector<uint32_t> n, m;
    std::vector<size_t> aoff, boff;  // offsets of a and b in d_seq
    std::vector<uint32_t> order;     // the planner's order: packed pairs by (g, |a|), then strip pairs by |a|
    DeviceBuf d_seq, d_cost;
    Plan<PairT, WaveT> fwd;
    double trace_chunks = 0;
    struct Tiled {
        double chunks = 0, rounds = 0, tile_jobs = 0, refill_cells = 0, chunk_bytes_max = 0;
    } tiled;  // the last align_tiled()
};

// Pair p of the batch, H = rows_of(|b|), without codes.
template <class T>
typename T::Pair make_pair(const typename T::Batch& ab, uint32_t p, uint32_t H) {
    typename T::Pair Q;
    std::memset(&Q, 0, sizeof Q);
    Q.a = ab.d_seq.template as<uint8_t>() + ab.aoff[p];
    Q.b = ab.d_seq.template as<uint8_t>() + ab.boff[p];
    Q.n = ab.n[p];
    Q.m = ab.m[p];
    Q.H = H;
    Q.out = p;
    return Q;
}

// The waves of affine_plan::plan_waves over `ids` as the kernels' records, uploaded.  `base`: where the pairs' codes (Keep::kCodes) or
// column checkpoints (Keep::kCkpt, tile_cols columns apart) go; the boundary rows are allocated here.
template <class T, class PlanT>
int make_plan(const typename T::Batch& ab, const std::vector<uint32_t>& ids, PlanT& P, Keep keep, uint8_t* base, hipStream_t s, uint32_t tile_cols = 0) {
    P.at = affine_plan::plan_waves(T::kLayout, ab.n, ab.m, ids, keep, tile_cols);
    const affine_plan::Waves& W = P.at;
    if (!P.d_bnd.alloc(std::max<size_t>(W.bnd_vals * T::kLayout.bnd_bytes, 16))) return PA_E_HIP;
    P.pairs.reserve(W.pairs.size());
    P.waves.reserve(W.waves.size());
    for (const affine_plan::PairSlot& q : W.pairs) {
        typename T::Pair Q = make_pair<T>(ab, q.id, q.H);
        if (keep != Keep::kNone) Q.codes = base + q.data_off;
        P.pairs.push_back(Q);
    }
    for (const affine_plan::WaveSlot& w : W.waves) {
        typename PlanT::Wave V;
        std::memset(&V, 0, sizeof V);
        V.first = w.first;
        V.np = w.np;
        V.lg = w.lg;
        V.strips = w.strips;
        V.nmax = w.nmax;
        V.tile_cols = tile_cols;
        if (w.bnd_off != SIZE_MAX) V.bnd = reinterpret_cast<decltype(V.bnd)>(P.d_bnd.template as<uint8_t>() + w.bnd_off);
        P.waves.push_back(V);
    }
    if (!upload(P.d_waves, P.waves.data(), P.waves.size() * sizeof(P.waves[0]), s) ||
        !upload(P.d_pairs, P.pairs.data(), P.pairs.size() * sizeof(typename T::Pair), s))
        return PA_E_HIP;
    return 0;
}

// The tail of *_batch_create, after the cost model has been checked: the pairs' own checks given the largest edge cost, then the batch
// with its sequences uploaded, the planner's order and the plan of run().
template <class T, class Costs>
typename T::Batch* create(const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b, const size_t* b_len, size_t npairs, int trace,
                          uint64_t max_edge, const Costs& C) {
    for (size_t p = 0; p < npairs; ++p) {
        if ((a_len[p] && !a[p]) || (b_len[p] && !b[p])) {
            set_error("%s_create: pair %zu: NULL sequence", T::kName, p);
            return nullptr;
        }
        if (a_len[p] >= (size_t(1) << 30) || b_len[p] >= (size_t(1) << 30) || ((uint64_t)a_len[p] + b_len[p] + 1) * max_edge >= (uint64_t(1) << 30)) {
            set_error("%s_create: pair %zu: (|a| + |b| + 1) * max edge cost = (%zu + %zu + 1) * %llu is not below 2^30", T::kName, p, a_len[p], b_len[p],
                      (unsigned long long)max_edge);
            return nullptr;
        }
    }
    if (!ensure_device()) return nullptr;
    typename T::Batch* ab = new (std::nothrow) typename T::Batch;
    if (!ab) {
        set_error("out of memory");
        return nullptr;
    }
    ab->C = C;
    ab->np = npairs;
    ab->trace = trace != 0;
    ab->n.resize(npairs);
    ab->m.resize(npairs);
    ab->aoff.resize(npairs);
    ab->boff.resize(npairs);
    std::vector<uint8_t> seq;
    for (size_t p = 0; p < npairs; ++p) {
        ab->n[p] = (uint32_t)a_len[p];
        ab->m[p] = (uint32_t)b_len[p];
        ab->aoff[p] = seq.size();
        seq.insert(seq.end(), a[p], a[p] + a_len[p]);
        ab->boff[p] = seq.size();
        seq.insert(seq.end(), b[p], b[p] + b_len[p]);
    }
    ab->order = affine_plan::planner_order(T::kLayout, ab->n, ab->m);
    hipStream_t s = 0;
    if (!upload(ab->d_seq, seq.data(), seq.size(), s) || !ab->d_cost.alloc(std::max<size_t>(npairs, 1) * 4) ||
        make_plan<T>(*ab, ab->order, ab->fwd, Keep::kNone, nullptr, s) != 0 || !hip_ok(hipStreamSynchronize(s), "sync")) {
        delete ab;
        return nullptr;
    }
    return ab;
}

// *_batch_align: the pairs in chunks whose traceback codes fit the budget; per chunk the fill, the walk of every pair, and the CIGARs.
template <class T>
int align(typename T::Batch* ab, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    using Walk = typename T::Walk;
    using WalkOut = typename T::WalkOut;
    if (!ab) return fail(PA_E_ARG, "%s_align: NULL batch", T::kName);
    if (forward_ms) *forward_ms = 0;
    if (trace_ms) *trace_ms = 0;
    if (cigar_out)
        for (size_t p = 0; p < ab->np; ++p) cigar_out[p] = nullptr;
    if (!ab->trace) return fail(PA_E_ARG, "%s_align: the batch was created without trace", T::kName);
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");  // (the traceback codes dominate a chunk)
    auto code_bytes = [&](uint32_t p) { return affine_plan::code_bytes_of(T::kLayout, ab->n[p], ab->m[p]); };
    for (size_t p = 0; p < ab->np; ++p)
        if (code_bytes((uint32_t)p) > budget)
            return fail(PA_E_ARG, "%s_align: pair %zu: %zu bytes of traceback codes exceed the budget of %zu bytes", T::kName, p, code_bytes((uint32_t)p),
                        budget);
    hipStream_t s = 0;
    std::vector<std::string> cigars(ab->np);
    std::vector<int64_t> starts(ab->np, 0);
    ab->trace_chunks = 0;
    float fwd_total = 0, trace_total = 0;
    DeviceBuf d_codes, d_ops, d_walk, d_wout;
    for (size_t c0 = 0, bytes; c0 < ab->np;) {
        const std::vector<uint32_t> ids = affine_plan::next_chunk(ab->order, c0, budget, code_bytes, &bytes);
        ab->trace_chunks += 1;
        if (!d_codes.reserve(std::max<size_t>(bytes, 16))) return PA_E_HIP;
        Plan<typename T::Pair, typename T::Wave> P;
        if (const int rc = make_plan<T>(*ab, ids, P, Keep::kCodes, d_codes.as<uint8_t>(), s)) return rc;
        std::vector<Walk> walks(P.pairs.size());
        const size_t ops_bytes = P.at.ops_bytes;
        if (!d_ops.reserve(std::max<size_t>(ops_bytes, 16))) return PA_E_HIP;
        for (size_t k = 0; k < P.pairs.size(); ++k) {
            const typename T::Pair& Q = P.pairs[k];
            Walk& w = walks[k];
            w.a = Q.a;
            w.b = Q.b;
            w.codes = Q.codes;
            w.ops = d_ops.as<uint8_t>() + P.at.pairs[k].ops_off;
            w.n = Q.n;
            w.m = Q.m;
            w.H = Q.H;
            w.cap = Q.n + Q.m;
            T::walk_extra(*ab, Q, w);
        }
        const int nw = (int)walks.size();
        Events ev;
        if (!ev.make() || !upload(d_walk, walks.data(), walks.size() * sizeof(Walk), s) || !d_wout.reserve(std::max<size_t>(nw * sizeof(WalkOut), 16)) ||
            !hip_ok(hipEventRecord(ev.e[0], s), "event") || !T::template launch<true>(*ab, P, s) || !hip_ok(hipEventRecord(ev.e[1], s), "event"))
            return PA_E_HIP;
        std::vector<WalkOut> wout(nw);
        std::vector<uint8_t> ops(ops_bytes);
        if (!T::launch_walk(*ab, d_walk.as<Walk>(), nw, d_wout.as<WalkOut>(), s) || !hip_ok(hipEventRecord(ev.e[2], s), "event") ||
            !hip_ok(hipMemcpyAsync(wout.data(), d_wout.ptr, nw * sizeof(WalkOut), hipMemcpyDeviceToHost, s), "D2H") ||
            (ops_bytes && !hip_ok(hipMemcpyAsync(ops.data(), d_ops.ptr, ops_bytes, hipMemcpyDeviceToHost, s), "D2H")) ||
            !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        float f = 0, t = 0;
        if (!hip_ok(hipEventElapsedTime(&f, ev.e[0], ev.e[1]), "hipEventElapsedTime") || !hip_ok(hipEventElapsedTime(&t, ev.e[1], ev.e[2]), "hipEventElapsedTime"))
            return PA_E_HIP;
        fwd_total += f;
        trace_total += t;
        for (size_t k = 0; k < P.pairs.size(); ++k) {
            const WalkOut& o = wout[k];
            if (o.status != 0)
                return fail(PA_E_INTERNAL, "%s_align: pair %u: %s", T::kName, P.pairs[k].out, o.status == 1 ? "bad traceback code" : "path longer than its buffer");
            cigars[P.pairs[k].out] = T::cigar_of(ops.data() + P.at.pairs[k].ops_off, o.nops);
            starts[P.pairs[k].out] = T::walk_start(o);
        }
        c0 += ids.size();
    }
    if (const int rc = T::finish(*ab, cost_out, s, &starts)) return rc;
    if (forward_ms) *forward_ms = fwd_total;
    if (trace_ms) *trace_ms = trace_total;
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

// One chunk of align_tiled: the checkpoint pass's plan with its row checkpoints, and where every pair (index k into plan.pairs) keeps
// its rest.
template <class T>
struct TiledChunk {
    Plan<typename T::Pair, typename T::Wave> plan;
    std::vector<const uint8_t*> ck;     // column checkpoints
    std::vector<const uint8_t*> rowck;  // row checkpoints: strip s at rowck + s (n + 1) values; nullptr for one strip
    std::vector<typename T::WalkState> st;
    std::vector<uint32_t> visits;
    DeviceBuf d_ck, d_tiles, d_ops, d_state, d_jobs, d_twaves;
};

// The chunk's buffers, every walk at (n, m, main), and the checkpoint pass.
template <class T>
int tiled_forward(typename T::Batch& ab, const std::vector<uint32_t>& ids, uint32_t C, TiledChunk<T>& ch, hipStream_t s, float* ms) {
    using WalkState = typename T::WalkState;
    size_t ck_bytes = 0;
    for (const uint32_t p : ids) ck_bytes += affine_plan::ckpt_bytes_of(T::kLayout, ab.n[p], ab.m[p], C);
    if (!ch.d_ck.alloc(std::max<size_t>(ck_bytes, 16))) return PA_E_HIP;
    if (const int rc = make_plan<T>(ab, ids, ch.plan, Keep::kCkpt, ch.d_ck.template as<uint8_t>(), s, C)) return rc;
    const size_t np = ch.plan.pairs.size();
    ch.ck.resize(np);
    ch.rowck.assign(np, nullptr);
    ch.st.resize(np);
    ch.visits.assign(np, 0);
    for (size_t k = 0; k < np; ++k) {
        const typename T::Pair& Q = ch.plan.pairs[k];
        ch.ck[k] = Q.codes;
        ch.st[k] = WalkState{(int32_t)Q.n, (int32_t)Q.m, 0, 0, 0, 0};
    }
    if (!ch.d_tiles.alloc(std::max<size_t>(ch.plan.at.tile_bytes, 16)) || !ch.d_ops.alloc(std::max<size_t>(ch.plan.at.ops_bytes, 16))) return PA_E_HIP;
    for (const auto& W : ch.plan.waves)
        if (W.strips > 1) ch.rowck[W.first] = reinterpret_cast<const uint8_t*>(W.bnd);
    if (!upload(ch.d_state, ch.st.data(), np * sizeof(WalkState), s)) return PA_E_HIP;
    return T::ckpt_pass(ab, ch, C, s, ms);
}

// The tile job of every unfinished pair, grouped into waves like the planner's (consecutive packed pairs of one width share a wave).
template <class T>
int tiled_jobs(typename T::Batch& ab, uint32_t C, TiledChunk<T>& ch, std::vector<typename T::TileJob>& jobs, std::vector<typename T::TileWave>& waves) {
    jobs.clear();
    waves.clear();
    for (size_t k = 0; k < ch.plan.pairs.size(); ++k) {
        const typename T::Pair& Q = ch.plan.pairs[k];
        const typename T::WalkState& S = ch.st[k];
        if (S.status != 0)
            return fail(PA_E_INTERNAL, "%s_align_tiled: pair %u: %s", T::kName, Q.out, S.status == 1 ? "bad traceback code" : "path longer than its buffer");
        if (T::walk_done(ab, S)) continue;
        const uint32_t visits_max = affine_plan::tile_visits_max(T::kLayout, Q.n, Q.m, C);
        if (S.i < 0 || S.j < 0 || (uint32_t)S.i > Q.n || (uint32_t)S.j > Q.m || S.layer < 0 || S.layer > T::kMaxLayer ||
            ++ch.visits[k] > visits_max + T::kVisitSlack)
            return fail(PA_E_INTERNAL, "%s_align_tiled: pair %u: the walk left its %u tiles at (%d, %d)", T::kName, Q.out, visits_max, S.i, S.j);
        const affine_plan::TileGeom G = affine_plan::tile_geom(T::kLayout, Q.n, Q.H, ch.plan.at.pairs[k].lg, C, (uint32_t)S.i, (uint32_t)S.j);
        typename T::TileJob J;
        std::memset(&J, 0, sizeof J);
        J.a = Q.a;
        J.b = Q.b;
        J.codes = ch.d_tiles.template as<uint8_t>() + ch.plan.at.pairs[k].tile_off;
        if (G.ct) J.left = reinterpret_cast<decltype(J.left)>(ch.ck[k] + G.left_off);
        if (G.ct) J.left0 = reinterpret_cast<decltype(J.left0)>(ch.ck[k] + G.left0_off);
        if (G.rt) J.above = reinterpret_cast<decltype(J.above)>(ch.rowck[k] + G.above_off);
        J.ops = ch.d_ops.template as<uint8_t>() + ch.plan.at.pairs[k].ops_off;
        J.state = ch.d_state.template as<typename T::WalkState>() + k;
        J.m = Q.m;
        J.Ht = G.Ht;
        J.rt = G.rt;
        J.c0 = G.c0;
        J.c1 = G.c1;
        J.row0 = G.row0;
        J.cap = Q.n + Q.m;
        J.rlast = G.rlast;
        if (waves.empty() || !affine_plan::joins_tile_wave(G, waves.back().lg, waves.back().np))
            waves.push_back(typename T::TileWave{(uint32_t)jobs.size(), 0, G.lg, 0});
        waves.back().np += 1;
        waves.back().steps = std::max(waves.back().steps, G.steps);
        jobs.push_back(J);
        ab.tiled.tile_jobs += 1;
        ab.tiled.refill_cells += G.refill_cells;
    }
    return 0;
}

// One round: re-fill every job's tile, walk every job's pair through it, and fetch where the walks stand.
template <class T>
int tiled_round(typename T::Batch& ab, TiledChunk<T>& ch, const std::vector<typename T::TileJob>& jobs, const std::vector<typename T::TileWave>& waves,
                Events& ev, hipStream_t s, float* refill_ms, float* walk_ms) {
    using TileJob = typename T::TileJob;
    using TileWave = typename T::TileWave;
    const int nj = (int)jobs.size(), nw = (int)waves.size();
    if (!ch.d_jobs.reserve(jobs.size() * sizeof(TileJob)) || !ch.d_twaves.reserve(waves.size() * sizeof(TileWave)) ||
        !hip_ok(hipMemcpyAsync(ch.d_jobs.ptr, jobs.data(), jobs.size() * sizeof(TileJob), hipMemcpyHostToDevice, s), "H2D") ||
        !hip_ok(hipMemcpyAsync(ch.d_twaves.ptr, waves.data(), waves.size() * sizeof(TileWave), hipMemcpyHostToDevice, s), "H2D") ||
        !hip_ok(hipEventRecord(ev.e[0], s), "event"))
        return PA_E_HIP;
    float f = 0, w = 0;
    if (!T::launch_tile_fill(ab, ch.d_twaves.template as<TileWave>(), nw, ch.d_jobs.template as<TileJob>(), s) ||
        !hip_ok(hipEventRecord(ev.e[1], s), "event") || !T::launch_tile_walk(ab, ch.d_jobs.template as<TileJob>(), nj, s) ||
        !hip_ok(hipEventRecord(ev.e[2], s), "event") ||
        !hip_ok(hipMemcpyAsync(ch.st.data(), ch.d_state.ptr, ch.st.size() * sizeof(typename T::WalkState), hipMemcpyDeviceToHost, s), "D2H") ||
        !hip_ok(hipStreamSynchronize(s), "sync") || !hip_ok(hipEventElapsedTime(&f, ev.e[0], ev.e[1]), "hipEventElapsedTime") ||
        !hip_ok(hipEventElapsedTime(&w, ev.e[1], ev.e[2]), "hipEventElapsedTime"))
        return PA_E_HIP;
    *refill_ms += f;
    *walk_ms += w;
    return 0;
}

// *_batch_align_tiled: the pairs in chunks whose checkpoints, tiles and ops fit the budget; per chunk the checkpoint pass, then rounds
// until every walk is done.
template <class T>
int align_tiled(typename T::Batch* ab, uint32_t tile_cols, int32_t* cost_out, char** cigar_out, float* forward_ms, float* refill_ms, float* walk_ms) {
    using namespace affine_plan;
    if (!ab) return fail(PA_E_ARG, "%s_align_tiled: NULL batch", T::kName);
    if (forward_ms) *forward_ms = 0;
    if (refill_ms) *refill_ms = 0;
    if (walk_ms) *walk_ms = 0;
    if (cigar_out)
        for (size_t p = 0; p < ab->np; ++p) cigar_out[p] = nullptr;
    if (!ab->trace) return fail(PA_E_ARG, "%s_align_tiled: the batch was created without trace", T::kName);
    if (tile_cols != 0 && (tile_cols < kTileColsMin || tile_cols > kTileColsMax))
        return fail(PA_E_ARG, "%s_align_tiled: tile_cols = %u outside [%u, %u] (0 = the default, %u)", T::kName, tile_cols, kTileColsMin, kTileColsMax,
                    kTileColsDefault);
    const uint32_t C = tile_cols ? tile_cols : kTileColsDefault;
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    auto tiled_bytes = [&](uint32_t p) { return tiled_bytes_of(T::kLayout, ab->n[p], ab->m[p], C); };
    for (size_t p = 0; p < ab->np; ++p)
        if (tiled_bytes((uint32_t)p) > budget)
            return fail(PA_E_ARG, "%s_align_tiled: pair %zu: %zu bytes of checkpoints, tile and ops exceed the budget of %zu bytes", T::kName, p,
                        tiled_bytes((uint32_t)p), budget);
    hipStream_t s = 0;
    std::vector<std::string> cigars(ab->np);
    std::vector<int64_t> starts(ab->np, 0);
    ab->tiled = {};
    T::begin_tiled(*ab);
    float fwd_total = 0, refill_total = 0, walk_total = 0;
    std::vector<typename T::TileJob> jobs;
    std::vector<typename T::TileWave> waves;
    for (size_t c0 = 0, bytes; c0 < ab->np;) {
        const std::vector<uint32_t> ids = next_chunk(ab->order, c0, budget, tiled_bytes, &bytes);
        ab->tiled.chunks += 1;
        ab->tiled.chunk_bytes_max = std::max(ab->tiled.chunk_bytes_max, (double)bytes);
        TiledChunk<T> ch;
        float f = 0;
        if (const int rc = tiled_forward<T>(*ab, ids, C, ch, s, &f)) return rc;
        fwd_total += f;
        Events ev;
        if (!ev.make()) return PA_E_HIP;
        for (;;) {  // ends: every round moves each unfinished pair into another tile, and tiled_jobs() bounds the tiles of a pair
            if (const int rc = tiled_jobs<T>(*ab, C, ch, jobs, waves)) return rc;
            if (jobs.empty()) break;
            ab->tiled.rounds += 1;
            if (const int rc = tiled_round<T>(*ab, ch, jobs, waves, ev, s, &refill_total, &walk_total)) return rc;
        }
        const size_t ops_bytes = ch.plan.at.ops_bytes;
        std::vector<uint8_t> ops(ops_bytes);
        if (ops_bytes && (!hip_ok(hipMemcpyAsync(ops.data(), ch.d_ops.ptr, ops_bytes, hipMemcpyDeviceToHost, s), "D2H") ||
                          !hip_ok(hipStreamSynchronize(s), "sync")))
            return PA_E_HIP;
        for (size_t k = 0; k < ch.plan.pairs.size(); ++k) {
            cigars[ch.plan.pairs[k].out] = T::cigar_of(ops.data() + ch.plan.at.pairs[k].ops_off, ch.st[k].nops);
            starts[ch.plan.pairs[k].out] = ch.st[k].i;
        }
        c0 += ids.size();
    }
    if (const int rc = T::finish(*ab, cost_out, s, &starts)) return rc;
    if (forward_ms) *forward_ms = fwd_total;
    if (refill_ms) *refill_ms = refill_total;
    if (walk_ms) *walk_ms = walk_total;
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

// ---- ends-free mode (set_free_ends, ends, last_row), the same for both batches ----
//
// The batch keeps `DeviceBuf d_end` (every pair's end, left there by the kernels' ENDS instantiations) and `EndsState ends`; the traits
// add
//   ends_flags(ab), set_ends_flags(ab, f)   the switches, kFreeStart | kFreeEnd, wherever the batch's kernels read them
//   launch_rows(ab, P, d_rows, d_off, s)    the cost-only ENDS kernel over a plan, which also stores the last rows (last_row())
// and finish() is costs_out<T>.

constexpr uint32_t kFreeStart = 1, kFreeEnd = 2;

// What *_batch_ends reports.
struct EndsState {
    bool valid = false;               // a run, align or align_tiled has succeeded under the current setting
    std::vector<int64_t> start, end;  // of that call
};

// Every pair's end after an ends-free pass (global mode: |a|, without a copy).
template <class T>
int fetch_ends(const typename T::Batch& ab, std::vector<int32_t>& end, hipStream_t s) {
    end.assign(ab.n.begin(), ab.n.end());
    if (ab.np == 0 || !T::ends_flags(ab)) return 0;
    if (!hip_ok(hipMemcpyAsync(end.data(), ab.d_end.ptr, ab.np * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    return 0;
}

// The costs of every pair, to the caller; the end of run(), align() and align_tiled().  Keeps what *_batch_ends reports: the ends, and
// the starts a traced call found (start; a cost-only run has none: -1 under a free start, else 0).
template <class T>
int costs_out(typename T::Batch& ab, int32_t* cost_out, hipStream_t s, const std::vector<int64_t>* start = nullptr) {
    ab.ends.valid = false;
    std::vector<int32_t> c(ab.np), e;
    if (ab.np && (!hip_ok(hipMemcpyAsync(c.data(), ab.d_cost.ptr, ab.np * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync")))
        return PA_E_HIP;
    if (const int rc = fetch_ends<T>(ab, e, s)) return rc;
    if (cost_out && ab.np) std::memcpy(cost_out, c.data(), ab.np * 4);
    ab.ends.end.assign(e.begin(), e.end());
    if (start) ab.ends.start = *start;
    else ab.ends.start.assign(ab.np, (T::ends_flags(ab) & kFreeStart) ? -1 : 0);
    ab.ends.valid = true;
    return 0;
}

// *_batch_set_free_ends.
template <class T>
int set_free_ends(typename T::Batch* ab, int free_start, int free_end) {
    if (!ab) return fail(PA_E_ARG, "%s_set_free_ends: NULL batch", T::kName);
    if ((free_start != 0 && free_start != 1) || (free_end != 0 && free_end != 1))
        return fail(PA_E_ARG, "%s_set_free_ends: free_start = %d, free_end = %d: each is 0 or 1", T::kName, free_start, free_end);
    if ((free_start || free_end) && !ab->d_end.reserve(std::max<size_t>(ab->np, 1) * 4)) return PA_E_HIP;
    T::set_ends_flags(*ab, (free_start ? kFreeStart : 0) | (free_end ? kFreeEnd : 0));
    ab->ends.valid = false;
    return 0;
}

// *_batch_ends.
template <class T>
int batch_ends(const typename T::Batch* ab, int64_t* start_out, int64_t* end_out) {
    if (!ab) return fail(PA_E_ARG, "%s_ends: NULL batch", T::kName);
    if (!ab->ends.valid) return fail(PA_E_ARG, "%s_ends: no run, align or align_tiled has succeeded under the current setting", T::kName);
    if (start_out && ab->np) std::memcpy(start_out, ab->ends.start.data(), ab->np * 8);
    if (end_out && ab->np) std::memcpy(end_out, ab->ends.end.data(), ab->np * 8);
    return 0;
}

// With a free end every walk of a tiled chunk starts at (end, m, main), the end the checkpoint pass found.
template <class T>
int seed_walks(typename T::Batch& ab, TiledChunk<T>& ch, hipStream_t s) {
    if (!(T::ends_flags(ab) & kFreeEnd)) return 0;
    const size_t np = ch.plan.pairs.size();
    std::vector<int32_t> end;
    if (const int rc = fetch_ends<T>(ab, end, s)) return rc;
    for (size_t k = 0; k < np; ++k) ch.st[k].i = end[ch.plan.pairs[k].out];
    if (!upload(ch.d_state, ch.st.data(), np * sizeof(typename T::WalkState), s) || !hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
    return 0;
}

// *_batch_last_row: a cost-only pass of its own over the pairs that are asked for, in chunks whose rows fit the budget.  (It leaves costs
// and ends of its chunks in d_cost and d_end, which every other call reads only right after its own pass.)
template <class T>
int last_row(typename T::Batch* ab, int32_t* out, const uint64_t* offsets) {
    if (!ab) return fail(PA_E_ARG, "%s_last_row: NULL batch", T::kName);
    if (ab->np == 0) return 0;
    if (!out || !offsets) return fail(PA_E_ARG, "%s_last_row: NULL array", T::kName);
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    std::vector<uint32_t> want;
    for (const uint32_t p : ab->order)
        if (offsets[p] != UINT64_MAX) {
            if (((size_t)ab->n[p] + 1) * 4 > budget)
                return fail(PA_E_ARG, "%s_last_row: pair %u: %zu bytes of last row exceed the budget of %zu bytes", T::kName, p, ((size_t)ab->n[p] + 1) * 4,
                            budget);
            want.push_back(p);
        }
    hipStream_t s = 0;
    DeviceBuf d_rows, d_off;
    if (!ab->d_end.reserve(ab->np * 4)) return PA_E_HIP;
    std::vector<uint64_t> off(ab->np);
    std::vector<int32_t> rows;
    for (size_t c0 = 0; c0 < want.size();) {
        std::fill(off.begin(), off.end(), UINT64_MAX);
        size_t c1 = c0, words = 0;
        while (c1 < want.size() && (c1 == c0 || (words + ab->n[want[c1]] + 1) * 4 <= budget)) {
            off[want[c1]] = words;
            words += (size_t)ab->n[want[c1]] + 1;
            ++c1;
        }
        const std::vector<uint32_t> ids(want.begin() + c0, want.begin() + c1);
        Plan<typename T::Pair, typename T::Wave> P;
        if (const int rc = make_plan<T>(*ab, ids, P, Keep::kNone, nullptr, s)) return rc;
        rows.resize(words);
        if (!d_rows.reserve(words * 4) || !upload(d_off, off.data(), off.size() * 8, s)) return PA_E_HIP;
        if (!T::launch_rows(*ab, P, d_rows.as<int32_t>(), d_off.as<uint64_t>(), s) ||
            !hip_ok(hipMemcpyAsync(rows.data(), d_rows.ptr, words * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        for (const uint32_t p : ids) std::memcpy(out + offsets[p], rows.data() + off[p], ((size_t)ab->n[p] + 1) * 4);
        c0 = c1;
    }
    return 0;
}

template <class BatchT>
void tiled_info(const BatchT* ab, double* chunks, double* rounds, double* tile_jobs, double* refill_cells, double* chunk_bytes_max) {
    if (chunks) *chunks = ab ? ab->tiled.chunks : 0;
    if (rounds) *rounds = ab ? ab->tiled.rounds : 0;
    if (tile_jobs) *tile_jobs = ab ? ab->tiled.tile_jobs : 0;
    if (refill_cells) *refill_cells = ab ? ab->tiled.refill_cells : 0;
    if (chunk_bytes_max) *chunk_bytes_max = ab ? ab->tiled.chunk_bytes_max : 0;
}

template <class BatchT>
void batch_info(const BatchT* ab, double* waves, double* packed_pairs, double* strip_pairs, double* lane_use, double* trace_chunks) {
    if (waves) *waves = ab ? (double)ab->fwd.waves.size() : 0;
    if (packed_pairs) *packed_pairs = ab ? (double)ab->fwd.at.packed : 0;
    if (strip_pairs) *strip_pairs = ab ? (double)ab->fwd.at.strip : 0;
    if (lane_use) *lane_use = ab && ab->fwd.at.slots > 0 ? ab->fwd.at.lanes / ab->fwd.at.slots : 0;
    if (trace_chunks) *trace_chunks = ab ? ab->trace_chunks : 0;
}

}  // namespace affine_host
}  // namespace pa
