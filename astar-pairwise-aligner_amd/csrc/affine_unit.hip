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
// The diagonal-transition route (run_dt, align_dt) is a unit of its own, affine_dt_unit.hip, which sees a batch through dt_view().
#include "pa_hip_internal.hpp"
#include "engine.hpp"
#include "affine_kernel.hpp"
#include "affine_chain_plan.hpp"
#include "affine_dt_view.hpp"
#include "../../include/pa_affine_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace pa;
using namespace pa::affine;

namespace {

constexpr uint32_t kMaxCost = 1000;
constexpr size_t kStripRows = 64 * kRows;  // rows of one strip

int seg_lg(size_t m) {  // log2 of the segment width: smallest g = 2^lg with g kRows >= m
    int lg = 0;
    while ((size_t(kRows) << lg) < m) ++lg;
    return lg;
}

// One launch's worth of waves over a subset of the pairs.
struct Plan {
    std::vector<Wave> waves;
    std::vector<Pair> pairs;
    size_t bnd_words = 0, code_bytes = 0;
    double lanes = 0, slots = 0;
    size_t packed = 0, strip = 0;
    DeviceBuf d_waves, d_pairs, d_bnd;
};

}  // namespace

struct pa_affine_batch {
    size_t np = 0;
    bool trace = false;
    Costs C{};
    std::vector<uint32_t> n, m;
    std::vector<size_t> aoff, boff;  // offsets of a and b in d_seq
    std::vector<uint32_t> order;     // the planner's order: packed pairs by (g, |a|), then strip pairs by |a|
    DeviceBuf d_seq, d_cost;
    Plan fwd;
    double trace_chunks = 0;
    struct {
        double chunks = 0, rounds = 0, tile_jobs = 0, refill_cells = 0, chunk_bytes_max = 0;
    } tiled;  // the last align_tiled()
    // The chained route (set_chain): the packed pairs keep a plan of their own, the others are listed in planner order.
    struct {
        bool on = false, built = false;
        std::vector<uint32_t> ids;  // pairs with |b| > 1024, in planner order
        Plan packed;                // the plan of the rest
        DeviceBuf d_pairs;          // Pair of every id
        DeviceBuf d_jobs, d_bnd, d_ticket_err;
        double pairs = 0, jobs = 0, chunks = 0, bnd_bytes_max = 0;  // the last chained pass
    } chain;
    // Ends-free mode (set_free_ends): the switches are C.ends, the kernels leave every pair's end in d_end.
    DeviceBuf d_end;
    struct {
        bool valid = false;               // a run, align or align_tiled has succeeded under the current setting
        std::vector<int64_t> start, end;  // of that call
    } ends;
    DtState* dt = nullptr;  // the diagonal-transition route's own state (affine_dt_unit.hip)
};

// What the diagonal-transition route (run_dt, align_dt: affine_dt_unit.hip) reads of a batch.
DtView pa::affine::dt_view(pa_affine_batch* ab) {
    static_assert(kDtAbsent == kInf, "an absent edge");
    const Costs& C = ab->C;
    const size_t seq_bytes = ab->np ? ab->boff[ab->np - 1] + ab->m[ab->np - 1] : 0;  // (b of the last pair ends d_seq)
    return DtView{ab->np, ab->trace, DtCosts{C.sub, C.ins, C.del, C.io, C.ie, C.dopen, C.de, C.ends}, ab->n.data(), ab->m.data(),
                  ab->aoff.data(), ab->boff.data(), ab->d_seq.as<uint8_t>(), seq_bytes, &ab->dt};
}

namespace {

size_t strips_of(uint32_t m) { return m <= kStripRows ? 1 : (m + kStripRows - 1) / kStripRows; }
size_t rows_of(uint32_t m) { return m <= kStripRows ? size_t(kRows) << seg_lg(m) : strips_of(m) * kStripRows; }  // H
size_t code_bytes_of(uint32_t n, uint32_t m) { return (((size_t)n + 1) * (rows_of(m) + 1) + 15) & ~size_t(15); }

// The tiled traceback ("Tiled traceback").  Column tiles of 1024 columns are as wide as the row tiles (a strip) are
// high: the row and the column checkpoints then cost the same |a| |b| / 128 bytes each, a tile of codes is 1 MiB, and a path near the
// diagonal crosses about as many column edges as row edges.
constexpr uint32_t kTileColsDefault = 1024, kTileColsMin = 64, kTileColsMax = 1u << 20;

size_t ckpt_cols_of(uint32_t n, uint32_t C) { return n ? (n - 1) / C : 0; }  // checkpointed columns C, 2C, .. < n
size_t tile_rows_of(uint32_t m) { return std::min(rows_of(m), kStripRows); }
size_t tile_cols_of(uint32_t n, uint32_t C) { return (size_t)std::min(n, C) + 1; }  // columns of the widest tile (column tile 0 has column 0 too)
size_t tile_bytes_of(uint32_t n, uint32_t m, uint32_t C) { return (tile_cols_of(n, C) * (tile_rows_of(m) + 1) + 15) & ~size_t(15); }
// Device bytes of one pair: row checkpoints, column checkpoints (row 0 included), one tile of codes, the ops.
size_t tiled_bytes_of(uint32_t n, uint32_t m, uint32_t C) {
    return (strips_of(m) - 1) * ((size_t)n + 1) * 8 + ckpt_cols_of(n, C) * (rows_of(m) + 1) * 8 + tile_bytes_of(n, m, C) + (size_t)n + m;
}
// Tiles a monotone path can visit: one more column tile or one more row tile per move.
uint32_t tile_visits_max(uint32_t n, uint32_t m, uint32_t C) {
    return (uint32_t)((n + (size_t)C - 1) / C + (std::max<uint32_t>(m, 1) + kStripRows - 1) / kStripRows);
}

// The CIGAR text of a walk's ops (recorded from the end backwards).
std::string cigar_of(const uint8_t* op, int32_t nops) {
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

// Pair p of the batch, without codes.
Pair make_pair(const pa_affine_batch& ab, uint32_t p) {
    Pair Q;
    std::memset(&Q, 0, sizeof Q);
    Q.a = ab.d_seq.as<uint8_t>() + ab.aoff[p];
    Q.b = ab.d_seq.as<uint8_t>() + ab.boff[p];
    Q.n = ab.n[p];
    Q.m = ab.m[p];
    Q.H = (uint32_t)rows_of(ab.m[p]);
    Q.out = p;
    return Q;
}

// Waves over `ids` (in planner order): 64 / g packed pairs of one width per wave, a wave per strip pair; then most expensive first.
// ck_base (the checkpoint pass of the tiled traceback, tile_cols columns apart): every pair gets its column checkpoints there, and
// every strip but the last a boundary row of its own.
int make_plan(const pa_affine_batch& ab, const std::vector<uint32_t>& ids, Plan& P, uint8_t* codes_base, hipStream_t s, uint64_t* ck_base = nullptr,
              uint32_t tile_cols = 0) {
    size_t ck_words = 0;
    std::vector<size_t> bnd_off;
    for (size_t x = 0; x < ids.size();) {
        const uint32_t p0 = ids[x];
        const bool packed = ab.m[p0] <= kStripRows;
        const int lg = packed ? seg_lg(ab.m[p0]) : 6;
        const size_t per = packed ? size_t(64) >> lg : 1;
        Wave W;
        std::memset(&W, 0, sizeof W);
        W.first = (uint32_t)P.pairs.size();
        W.lg = (uint32_t)lg;
        W.strips = (uint32_t)strips_of(ab.m[p0]);
        W.tile_cols = tile_cols;
        while (x < ids.size() && W.np < per) {
            const uint32_t p = ids[x];
            if ((ab.m[p] <= kStripRows) != packed || (packed && seg_lg(ab.m[p]) != lg)) break;
            ++x;
            Pair Q = make_pair(ab, p);
            if (codes_base) {
                Q.codes = codes_base + P.code_bytes;
                P.code_bytes += code_bytes_of(Q.n, Q.m);
            } else if (ck_base) {
                Q.codes = reinterpret_cast<uint8_t*>(ck_base + ck_words);
                ck_words += ckpt_cols_of(Q.n, tile_cols) * ((size_t)Q.H + 1);
            }
            P.pairs.push_back(Q);
            P.lanes += (double)((std::max<uint32_t>(Q.m, 1) + kRows - 1) / kRows);
            W.nmax = std::max(W.nmax, Q.n);
            ++W.np;
            (packed ? P.packed : P.strip) += 1;
        }
        P.slots += 64.0 * W.strips;
        bnd_off.push_back(W.strips > 1 ? P.bnd_words : SIZE_MAX);
        if (W.strips > 1) P.bnd_words += (ck_base ? size_t(W.strips) - 1 : 1) * ((size_t)W.nmax + 1);
        P.waves.push_back(W);
    }
    if (!P.d_bnd.alloc(std::max<size_t>(P.bnd_words * 8, 16))) return PA_E_HIP;
    for (size_t w = 0; w < P.waves.size(); ++w)
        if (bnd_off[w] != SIZE_MAX) P.waves[w].bnd = P.d_bnd.as<uint64_t>() + bnd_off[w];
    std::stable_sort(P.waves.begin(), P.waves.end(), [](const Wave& x, const Wave& y) {
        return (uint64_t)x.strips * (x.nmax + (1u << x.lg)) > (uint64_t)y.strips * (y.nmax + (1u << y.lg));
    });
    if (!upload(P.d_waves, P.waves.data(), P.waves.size() * sizeof(Wave), s) || !upload(P.d_pairs, P.pairs.data(), P.pairs.size() * sizeof(Pair), s))
        return PA_E_HIP;
    return 0;
}

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

struct Events {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
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

// The device jobs of a chain plan, chunk after chunk, every chunk's rows at `rows`.  Pair p of the plan is pair at[p] of the kernel's Pair
// array (p itself without `at`).
std::vector<ChainJob> chain_jobs_of(const affine_chain::Plan& cp, const std::vector<affine_chain::Shape>& shapes, uint64_t* rows,
                                    const std::vector<uint32_t>* at = nullptr) {
    std::vector<ChainJob> jobs;
    jobs.reserve(cp.jobs.size());
    for (const affine_chain::Job& q : cp.jobs) {
        const size_t S = affine_chain::strips_of(shapes[q.pair].m), w = affine_chain::row_words(shapes[q.pair].n);
        uint64_t* row0 = rows + cp.row_off[q.pair];
        ChainJob J;
        J.pair = at ? (*at)[q.pair] : q.pair;
        J.strip = q.strip;
        J.bnd_in = q.strip ? row0 + (size_t)(q.strip - 1) * w : nullptr;
        J.bnd_out = q.strip + 1 < S ? row0 + (size_t)q.strip * w : nullptr;
        jobs.push_back(J);
    }
    return jobs;
}

// One chained pass, a launch per chunk of the plan: ticket and error word cleared and the chunk's rows (at `rows`) set to all-ones on the
// stream, the kernel over the chunk's jobs at d_jobs (chain_jobs_of), and the copy of its error word to errs, for chain_check to read once
// the stream is synchronised.  Counts the pass in chain.*.
template <bool CKPT>
bool launch_chain(pa_affine_batch& ab, const affine_chain::Plan& cp, const ChainJob* d_jobs, const Pair* d_pairs, uint32_t tile_cols, void* rows,
                  std::vector<uint32_t>& errs, hipStream_t s) {
    uint32_t* te = ab.chain.d_ticket_err.as<uint32_t>();
    errs.assign(cp.chunks.size(), 0);
    for (size_t k = 0; k < cp.chunks.size(); ++k) {
        const affine_chain::Chunk& c = cp.chunks[k];
        if (!hip_ok(hipMemsetAsync(te, 0, 8, s), "hipMemsetAsync") || (c.words && !hip_ok(hipMemsetAsync(rows, 0xFF, c.words * 8, s), "hipMemsetAsync")))
            return false;
        const int grid = (int)((c.njobs + kBlockWaves - 1) / kBlockWaves);
        if (ab.C.ends)
            hipLaunchKernelGGL((affine_chain_kernel<CKPT, true>), dim3(grid), dim3(64 * kBlockWaves), 0, s, d_jobs + c.first_job, (int)c.njobs, d_pairs, ab.C,
                               tile_cols, te, ab.d_cost.as<int32_t>(), ends_of(ab));
        else
            hipLaunchKernelGGL((affine_chain_kernel<CKPT, false>), dim3(grid), dim3(64 * kBlockWaves), 0, s, d_jobs + c.first_job, (int)c.njobs, d_pairs, ab.C,
                               tile_cols, te, ab.d_cost.as<int32_t>(), Ends{});
        if (!hip_ok(hipGetLastError(), CKPT ? "affine_chain_kernel<CKPT> launch" : "affine_chain_kernel launch") ||
            !hip_ok(hipMemcpyAsync(&errs[k], te + 1, 4, hipMemcpyDeviceToHost, s), "D2H"))
            return false;
    }
    ab.chain.pairs += (double)cp.row_off.size();
    ab.chain.jobs += (double)cp.jobs.size();
    ab.chain.chunks += (double)cp.chunks.size();
    ab.chain.bnd_bytes_max = std::max(ab.chain.bnd_bytes_max, (double)cp.words_max * 8);
    return true;
}

int chain_check(const char* fn, const std::vector<uint32_t>& errs) {
    uint32_t err = 0;
    for (const uint32_t e : errs)
        if (e) err = e;
    if (!err) return 0;
    return fail(PA_E_INTERNAL, "%s: chained route: a strip never received its boundary row (device spin timeout, err=%u); no result of this call is valid", fn,
                err);
}

// What set_chain(1) needs once: the chained pairs, their Pair array and the plan of the packed rest.
int chain_build(pa_affine_batch& ab, hipStream_t s) {
    if (ab.chain.built) return 0;
    std::vector<uint32_t> rest;
    ab.chain.ids.clear();  // (an earlier attempt may have failed half-way)
    for (const uint32_t p : ab.order) (ab.m[p] > kStripRows ? ab.chain.ids : rest).push_back(p);
    std::vector<Pair> pairs;
    for (const uint32_t p : ab.chain.ids) pairs.push_back(make_pair(ab, p));
    if (!upload(ab.chain.d_pairs, pairs.data(), pairs.size() * sizeof(Pair), s) || !ab.chain.d_ticket_err.alloc(16)) return PA_E_HIP;
    if (!ab.chain.ids.empty())  // (without chained pairs run() keeps the batch's own plan)
        if (const int rc = make_plan(ab, rest, ab.chain.packed, nullptr, s)) return rc;
    if (!hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
    ab.chain.built = true;
    return 0;
}

// run() with chaining on and pairs to chain: the packed pairs' launch, then the chained pairs in chunks whose boundary rows fit the budget.
int run_chained(pa_affine_batch& ab, Events& ev, hipStream_t s) {
    std::vector<affine_chain::Shape> shapes;
    for (const uint32_t p : ab.chain.ids) shapes.push_back(affine_chain::Shape{ab.n[p], ab.m[p]});
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    const affine_chain::Plan cp = affine_chain::plan(shapes, budget);
    if (cp.refused >= 0)
        return fail(PA_E_ARG, "pa_affine_batch_run: pair %u: %zu bytes of boundary rows of the chained route exceed the budget of %zu bytes",
                    ab.chain.ids[(size_t)cp.refused], affine_chain::pair_words(shapes[(size_t)cp.refused]) * 8, budget);
    if (!ab.chain.d_bnd.reserve(std::max<size_t>(cp.words_max * 8, 16))) return PA_E_HIP;
    const std::vector<ChainJob> jobs = chain_jobs_of(cp, shapes, ab.chain.d_bnd.as<uint64_t>());
    std::vector<uint32_t> errs;
    if (!ab.chain.d_jobs.reserve(jobs.size() * sizeof(ChainJob)) ||
        !hip_ok(hipMemcpyAsync(ab.chain.d_jobs.ptr, jobs.data(), jobs.size() * sizeof(ChainJob), hipMemcpyHostToDevice, s), "H2D") ||
        !hip_ok(hipStreamSynchronize(s), "sync") ||  // (jobs is pageable memory of this call)
        !hip_ok(hipEventRecord(ev.e[0], s), "event") || !launch<false>(ab, ab.chain.packed, s) ||
        !launch_chain<false>(ab, cp, ab.chain.d_jobs.as<ChainJob>(), ab.chain.d_pairs.as<Pair>(), 0, ab.chain.d_bnd.ptr, errs, s) ||
        !hip_ok(hipEventRecord(ev.e[1], s), "event") || !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    return chain_check("pa_affine_batch_run", errs);
}

// Every pair's end after an ends-free pass (global mode: |a|, without a copy).
int fetch_ends(const pa_affine_batch& ab, std::vector<int32_t>& end, hipStream_t s) {
    end.assign(ab.n.begin(), ab.n.end());
    if (ab.np == 0 || !ab.C.ends) return 0;
    if (!hip_ok(hipMemcpyAsync(end.data(), ab.d_end.ptr, ab.np * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    return 0;
}

// The costs of every pair, to the caller; the end of run(), align() and align_tiled().  Keeps what pa_affine_batch_ends reports: the ends,
// and the starts a traced call found (start; a cost-only run has none: -1 under a free start, else 0).
int costs_out(pa_affine_batch& ab, int32_t* cost_out, hipStream_t s, const std::vector<int64_t>* start = nullptr) {
    ab.ends.valid = false;
    std::vector<int32_t> c(ab.np), e;
    if (ab.np && (!hip_ok(hipMemcpyAsync(c.data(), ab.d_cost.ptr, ab.np * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync")))
        return PA_E_HIP;
    if (const int rc = fetch_ends(ab, e, s)) return rc;
    if (cost_out && ab.np) std::memcpy(cost_out, c.data(), ab.np * 4);
    ab.ends.end.assign(e.begin(), e.end());
    if (start) ab.ends.start = *start;
    else ab.ends.start.assign(ab.np, (ab.C.ends & kFreeStart) ? -1 : 0);
    ab.ends.valid = true;
    return 0;
}

// The next chunk of align() and align_tiled(): the pairs ab.order[c0 .. c1), as many as fit the budget by size_of(pair) and at least one;
// *bytes is their sum.
template <class SizeOf>
std::vector<uint32_t> next_chunk(const pa_affine_batch& ab, size_t c0, size_t budget, SizeOf size_of, size_t* bytes) {
    size_t c1 = c0;
    *bytes = 0;
    while (c1 < ab.np && (c1 == c0 || *bytes + size_of(ab.order[c1]) <= budget)) *bytes += size_of(ab.order[c1]), ++c1;
    return std::vector<uint32_t>(ab.order.begin() + c0, ab.order.begin() + c1);
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
    for (size_t p = 0; p < npairs; ++p) {
        if ((a_len[p] && !a[p]) || (b_len[p] && !b[p])) {
            set_error("pa_affine_batch_create: pair %zu: NULL sequence", p);
            return nullptr;
        }
        if (a_len[p] >= (size_t(1) << 30) || b_len[p] >= (size_t(1) << 30) || ((uint64_t)a_len[p] + b_len[p] + 1) * max_edge >= (uint64_t(1) << 30)) {
            set_error("pa_affine_batch_create: pair %zu: (|a| + |b| + 1) * max edge cost = (%zu + %zu + 1) * %llu is not below 2^30", p, a_len[p],
                      b_len[p], (unsigned long long)max_edge);
            return nullptr;
        }
    }
    if (!ensure_device()) return nullptr;
    pa_affine_batch* ab = new (std::nothrow) pa_affine_batch;
    if (!ab) {
        set_error("out of memory");
        return nullptr;
    }
    auto cost = [](int32_t c) { return c ? (uint32_t)c : kInf; };
    ab->C.sub = cost(cm->sub);
    ab->C.ins = cost(cm->ins);
    ab->C.del = cost(cm->del);
    ab->C.io = cost(cm->ins_open);
    ab->C.ie = cost(cm->ins_extend);
    ab->C.dopen = cost(cm->del_open);
    ab->C.de = cost(cm->del_extend);
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
    ab->order.resize(npairs);
    for (size_t p = 0; p < npairs; ++p) ab->order[p] = (uint32_t)p;
    std::stable_sort(ab->order.begin(), ab->order.end(), [&](uint32_t x, uint32_t y) {
        const int gx = ab->m[x] <= kStripRows ? seg_lg(ab->m[x]) : 7, gy = ab->m[y] <= kStripRows ? seg_lg(ab->m[y]) : 7;
        return gx != gy ? gx < gy : ab->n[x] < ab->n[y];
    });
    hipStream_t s = 0;
    if (!upload(ab->d_seq, seq.data(), seq.size(), s) || !ab->d_cost.alloc(std::max<size_t>(npairs, 1) * 4) ||
        make_plan(*ab, ab->order, ab->fwd, nullptr, s) != 0 || !hip_ok(hipStreamSynchronize(s), "sync")) {
        delete ab;
        return nullptr;
    }
    return ab;
}

extern "C" int pa_affine_batch_run(pa_affine_batch* ab, int32_t* cost_out, float* kernel_ms) {
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_run: NULL batch");
    if (kernel_ms) *kernel_ms = 0;
    hipStream_t s = 0;
    if (ab->np == 0) return costs_out(*ab, cost_out, s);  // (nothing to copy: the call counts for pa_affine_batch_ends)
    Events ev;
    if (!ev.make()) return PA_E_HIP;
    if (ab->chain.on) ab->chain.pairs = ab->chain.jobs = ab->chain.chunks = ab->chain.bnd_bytes_max = 0;
    if (ab->chain.on && !ab->chain.ids.empty()) {
        if (const int rc = run_chained(*ab, ev, s)) return rc;
    } else if (!hip_ok(hipEventRecord(ev.e[0], s), "event") || !launch<false>(*ab, ab->fwd, s) || !hip_ok(hipEventRecord(ev.e[1], s), "event"))
        return PA_E_HIP;
    if (const int rc = costs_out(*ab, cost_out, s)) return rc;
    if (kernel_ms && !hip_ok(hipEventElapsedTime(kernel_ms, ev.e[0], ev.e[1]), "hipEventElapsedTime")) return PA_E_HIP;
    return 0;
}

extern "C" int pa_affine_batch_align(pa_affine_batch* ab, int32_t* cost_out, char** cigar_out, float* forward_ms, float* trace_ms) {
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_align: NULL batch");
    if (forward_ms) *forward_ms = 0;
    if (trace_ms) *trace_ms = 0;
    if (cigar_out)
        for (size_t p = 0; p < ab->np; ++p) cigar_out[p] = nullptr;
    if (!ab->trace) return fail(PA_E_ARG, "pa_affine_batch_align: the batch was created without trace");
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");  // (the traceback codes dominate a chunk)
    for (size_t p = 0; p < ab->np; ++p)
        if (code_bytes_of(ab->n[p], ab->m[p]) > budget)
            return fail(PA_E_ARG, "pa_affine_batch_align: pair %zu: %zu bytes of traceback codes exceed the budget of %zu bytes", p,
                        code_bytes_of(ab->n[p], ab->m[p]), budget);
    hipStream_t s = 0;
    std::vector<std::string> cigars(ab->np);
    std::vector<int64_t> starts(ab->np, 0);
    ab->trace_chunks = 0;
    float fwd_total = 0, trace_total = 0;
    DeviceBuf d_codes, d_ops, d_walk, d_wout;
    for (size_t c0 = 0, bytes; c0 < ab->np;) {
        const std::vector<uint32_t> ids = next_chunk(*ab, c0, budget, [&](uint32_t p) { return code_bytes_of(ab->n[p], ab->m[p]); }, &bytes);
        ab->trace_chunks += 1;
        if (!d_codes.reserve(std::max<size_t>(bytes, 16))) return PA_E_HIP;
        Plan P;
        if (const int rc = make_plan(*ab, ids, P, d_codes.as<uint8_t>(), s)) return rc;
        std::vector<Walk> walks(P.pairs.size());
        size_t ops_bytes = 0;
        std::vector<size_t> ops_off(P.pairs.size());
        for (size_t k = 0; k < P.pairs.size(); ++k) {
            ops_off[k] = ops_bytes;
            ops_bytes += (size_t)P.pairs[k].n + P.pairs[k].m;
        }
        if (!d_ops.reserve(std::max<size_t>(ops_bytes, 16))) return PA_E_HIP;
        for (size_t k = 0; k < P.pairs.size(); ++k) {
            const Pair& Q = P.pairs[k];
            Walk& w = walks[k];
            w.a = Q.a;
            w.b = Q.b;
            w.codes = Q.codes;
            w.ops = d_ops.as<uint8_t>() + ops_off[k];
            w.n = Q.n;
            w.m = Q.m;
            w.H = Q.H;
            w.cap = Q.n + Q.m;
            w.out = Q.out;
            w.free_start = ab->C.ends & kFreeStart;
        }
        const int nw = (int)walks.size();
        Events ev;
        if (!ev.make() || !upload(d_walk, walks.data(), walks.size() * sizeof(Walk), s) || !d_wout.reserve(std::max<size_t>(nw * sizeof(WalkOut), 16)) ||
            !hip_ok(hipEventRecord(ev.e[0], s), "event") || !launch<true>(*ab, P, s) || !hip_ok(hipEventRecord(ev.e[1], s), "event"))
            return PA_E_HIP;
        hipLaunchKernelGGL(affine_walk_kernel, dim3((nw + 63) / 64), dim3(64), 0, s, d_walk.as<Walk>(), nw, d_wout.as<WalkOut>(),
                           (ab->C.ends & kFreeEnd) ? ab->d_end.as<int32_t>() : nullptr);
        std::vector<WalkOut> wout(nw);
        std::vector<uint8_t> ops(ops_bytes);
        if (!hip_ok(hipGetLastError(), "affine_walk_kernel launch") || !hip_ok(hipEventRecord(ev.e[2], s), "event") ||
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
                return fail(PA_E_INTERNAL, "pa_affine_batch_align: pair %u: %s", P.pairs[k].out, o.status == 1 ? "bad traceback code" : "path longer than its buffer");
            cigars[P.pairs[k].out] = cigar_of(ops.data() + ops_off[k], o.nops);
            starts[P.pairs[k].out] = o.start;
        }
        c0 += ids.size();
    }
    if (const int rc = costs_out(*ab, cost_out, s, &starts)) return rc;
    if (forward_ms) *forward_ms = fwd_total;
    if (trace_ms) *trace_ms = trace_total;
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

namespace {

// One chunk of align_tiled: the forward plan with its row checkpoints, and where every pair (index k into plan.pairs) keeps its rest.
struct TiledChunk {
    Plan plan;
    std::vector<const uint64_t*> ck;     // column checkpoints (affine_kernel.hpp, CKPT)
    std::vector<const uint64_t*> rowck;  // row checkpoints: strip s at rowck + s (n + 1); nullptr for one strip
    std::vector<size_t> tile_off, ops_off;
    size_t ops_bytes = 0;
    std::vector<WalkState> st;
    std::vector<uint32_t> visits;
    DeviceBuf d_ck, d_tiles, d_ops, d_state, d_jobs, d_twaves;
    DeviceBuf d_pwaves, d_cjobs;  // chained: the plan's one-strip waves, and the chain jobs of the others
};

// The chunk's buffers, the checkpoint pass, and every walk at (n, m, main) -- with a free end at (end, m, main).
int tiled_forward(pa_affine_batch& ab, const std::vector<uint32_t>& ids, uint32_t C, TiledChunk& ch, hipStream_t s, float* ms) {
    Plan& P = ch.plan;
    size_t ck_words = 0;
    for (const uint32_t p : ids) ck_words += ckpt_cols_of(ab.n[p], C) * (rows_of(ab.m[p]) + 1);
    if (!ch.d_ck.alloc(std::max<size_t>(ck_words * 8, 16))) return PA_E_HIP;
    if (const int rc = make_plan(ab, ids, P, nullptr, s, ch.d_ck.as<uint64_t>(), C)) return rc;
    const size_t np = P.pairs.size();
    ch.ck.resize(np);
    ch.rowck.assign(np, nullptr);
    ch.tile_off.resize(np);
    ch.ops_off.resize(np);
    ch.st.resize(np);
    ch.visits.assign(np, 0);
    size_t tile_bytes = 0;
    for (size_t k = 0; k < np; ++k) {
        const Pair& Q = P.pairs[k];
        ch.ck[k] = reinterpret_cast<const uint64_t*>(Q.codes);
        ch.tile_off[k] = tile_bytes;
        tile_bytes += tile_bytes_of(Q.n, Q.m, C);
        ch.ops_off[k] = ch.ops_bytes;
        ch.ops_bytes += (size_t)Q.n + Q.m;
        ch.st[k] = WalkState{(int32_t)Q.n, (int32_t)Q.m, 0, 0, 0, 0};
    }
    if (!ch.d_tiles.alloc(std::max<size_t>(tile_bytes, 16)) || !ch.d_ops.alloc(std::max<size_t>(ch.ops_bytes, 16))) return PA_E_HIP;
    for (const Wave& W : P.waves)
        if (W.strips > 1) ch.rowck[W.first] = W.bnd;
    Events ev;
    if (!ev.make() || !upload(ch.d_state, ch.st.data(), np * sizeof(WalkState), s)) return PA_E_HIP;
    const Wave* d_waves = P.d_waves.as<Wave>();
    size_t nwaves = P.waves.size();
    affine_chain::Plan cp;
    if (ab.chain.on) {  // the strip pairs leave the plan's launch for the chained one; their rows stay where make_plan put them
        std::vector<Wave> one;
        std::vector<affine_chain::Shape> shapes;
        std::vector<uint32_t> at;  // index into P.pairs
        for (const Wave& W : P.waves)
            if (W.strips == 1) one.push_back(W);
        for (size_t k = 0; k < np; ++k)  // (P.pairs keeps the order of ids; the waves are sorted by cost)
            if (P.pairs[k].m > kStripRows) {
                shapes.push_back(affine_chain::Shape{P.pairs[k].n, P.pairs[k].m});
                at.push_back((uint32_t)k);
            }
        cp = affine_chain::plan(shapes, SIZE_MAX);  // (this chunk was cut by tiled_bytes_of, which counts the rows)
        for (size_t x = 0; x < shapes.size(); ++x)
            if (cp.chunks.size() != 1 || ch.rowck[at[x]] != P.d_bnd.as<uint64_t>() + cp.row_off[x] || cp.words_max != P.bnd_words)
                return fail(PA_E_INTERNAL, "pa_affine_batch_align_tiled: chained route: the planner and the checkpoint plan disagree on pair %u's rows",
                            P.pairs[at[x]].out);
        const std::vector<ChainJob> cjobs = chain_jobs_of(cp, shapes, P.d_bnd.as<uint64_t>(), &at);
        if (!upload(ch.d_pwaves, one.data(), one.size() * sizeof(Wave), s) || !upload(ch.d_cjobs, cjobs.data(), cjobs.size() * sizeof(ChainJob), s) ||
            !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        d_waves = ch.d_pwaves.as<Wave>();
        nwaves = one.size();
    }
    std::vector<uint32_t> errs;
    if (!hip_ok(hipEventRecord(ev.e[0], s), "event") || !launch<false, true>(ab, d_waves, nwaves, P.d_pairs.as<Pair>(), s) ||
        !launch_chain<true>(ab, cp, ch.d_cjobs.as<ChainJob>(), P.d_pairs.as<Pair>(), C, P.d_bnd.ptr, errs, s) ||
        !hip_ok(hipEventRecord(ev.e[1], s), "event") || !hip_ok(hipStreamSynchronize(s), "sync") ||
        !hip_ok(hipEventElapsedTime(ms, ev.e[0], ev.e[1]), "hipEventElapsedTime"))
        return PA_E_HIP;
    if (const int rc = chain_check("pa_affine_batch_align_tiled", errs)) return rc;
    if (ab.C.ends & kFreeEnd) {  // every walk starts at (end, m, main), the end the checkpoint pass found
        std::vector<int32_t> end;
        if (const int rc = fetch_ends(ab, end, s)) return rc;
        for (size_t k = 0; k < np; ++k) ch.st[k].i = end[P.pairs[k].out];
        if (!upload(ch.d_state, ch.st.data(), np * sizeof(WalkState), s) || !hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
    }
    return 0;
}

// The tile job of every unfinished pair, grouped into waves like the planner's (consecutive packed pairs of one width share a wave).
int tiled_jobs(pa_affine_batch& ab, uint32_t C, TiledChunk& ch, std::vector<TileJob>& jobs, std::vector<TileWave>& waves) {
    jobs.clear();
    waves.clear();
    for (size_t k = 0; k < ch.plan.pairs.size(); ++k) {
        const Pair& Q = ch.plan.pairs[k];
        const WalkState& S = ch.st[k];
        if (S.status != 0)
            return fail(PA_E_INTERNAL, "pa_affine_batch_align_tiled: pair %u: %s", Q.out, S.status == 1 ? "bad traceback code" : "path longer than its buffer");
        if (S.j == 0 && S.layer == 0 && (S.i == 0 || (ab.C.ends & kFreeStart))) continue;  // walk_done
        if (S.i < 0 || S.j < 0 || (uint32_t)S.i > Q.n || (uint32_t)S.j > Q.m || ++ch.visits[k] > tile_visits_max(Q.n, Q.m, C) + 1)
            return fail(PA_E_INTERNAL, "pa_affine_batch_align_tiled: pair %u: the walk left its %u tiles at (%d, %d)", Q.out,
                        tile_visits_max(Q.n, Q.m, C), S.i, S.j);
        const uint32_t ct = S.i ? ((uint32_t)S.i - 1) / C : 0, rt = S.j ? ((uint32_t)S.j - 1) / (uint32_t)kStripRows : 0;
        TileJob J;
        std::memset(&J, 0, sizeof J);
        J.a = Q.a;
        J.b = Q.b;
        J.codes = ch.d_tiles.as<uint8_t>() + ch.tile_off[k];
        J.left = ct ? ch.ck[k] + (size_t)(ct - 1) * Q.H + (size_t)rt * kStripRows : nullptr;
        J.left0 = ct ? ch.ck[k] + ckpt_cols_of(Q.n, C) * Q.H + (ct - 1) : nullptr;
        J.above = rt ? ch.rowck[k] + (size_t)(rt - 1) * ((size_t)Q.n + 1) : nullptr;
        J.ops = ch.d_ops.as<uint8_t>() + ch.ops_off[k];
        J.state = ch.d_state.as<WalkState>() + k;
        J.m = Q.m;
        J.Ht = (uint32_t)tile_rows_of(Q.m);
        J.rt = rt;
        J.c0 = ct * C;
        J.c1 = (uint32_t)S.i;
        J.row0 = (uint32_t)(tile_cols_of(Q.n, C) * J.Ht);
        J.cap = Q.n + Q.m;
        J.rlast = S.j ? ((uint32_t)S.j - 1 - rt * (uint32_t)kStripRows) / kRows : 0;
        const uint32_t cols = J.c1 - (J.c0 ? J.c0 + 1 : 0) + 1, steps = cols + J.rlast;
        const bool packed = Q.m <= kStripRows;
        const uint32_t lg = packed ? (uint32_t)seg_lg(Q.m) : 6;
        if (waves.empty() || !packed || waves.back().lg != lg || waves.back().np == (64u >> lg))
            waves.push_back(TileWave{(uint32_t)jobs.size(), 0, lg, 0});
        waves.back().np += 1;
        waves.back().steps = std::max(waves.back().steps, steps);
        jobs.push_back(J);
        ab.tiled.tile_jobs += 1;
        ab.tiled.refill_cells += (double)cols * kRows * (J.rlast + 1);
    }
    return 0;
}

// One round: re-fill every job's tile, walk every job's pair through it, and fetch where the walks stand.
int tiled_round(pa_affine_batch& ab, TiledChunk& ch, const std::vector<TileJob>& jobs, const std::vector<TileWave>& waves, Events& ev, hipStream_t s,
                float* refill_ms, float* walk_ms) {
    const int nj = (int)jobs.size(), nw = (int)waves.size();
    if (!ch.d_jobs.reserve(jobs.size() * sizeof(TileJob)) || !ch.d_twaves.reserve(waves.size() * sizeof(TileWave)) ||
        !hip_ok(hipMemcpyAsync(ch.d_jobs.ptr, jobs.data(), jobs.size() * sizeof(TileJob), hipMemcpyHostToDevice, s), "H2D") ||
        !hip_ok(hipMemcpyAsync(ch.d_twaves.ptr, waves.data(), waves.size() * sizeof(TileWave), hipMemcpyHostToDevice, s), "H2D") ||
        !hip_ok(hipEventRecord(ev.e[0], s), "event"))
        return PA_E_HIP;
    const bool fs = ab.C.ends & kFreeStart;
    hipLaunchKernelGGL(fs ? affine_tile_kernel<true> : affine_tile_kernel<false>, dim3((nw + kBlockWaves - 1) / kBlockWaves), dim3(64 * kBlockWaves), 0, s,
                       ch.d_twaves.as<TileWave>(), nw, ch.d_jobs.as<TileJob>(), ab.C);
    if (!hip_ok(hipGetLastError(), "affine_tile_kernel launch") || !hip_ok(hipEventRecord(ev.e[1], s), "event")) return PA_E_HIP;
    hipLaunchKernelGGL(affine_tile_walk_kernel, dim3((nj + 63) / 64), dim3(64), 0, s, ch.d_jobs.as<TileJob>(), nj, fs ? 1 : 0);
    float f = 0, w = 0;
    if (!hip_ok(hipGetLastError(), "affine_tile_walk_kernel launch") || !hip_ok(hipEventRecord(ev.e[2], s), "event") ||
        !hip_ok(hipMemcpyAsync(ch.st.data(), ch.d_state.ptr, ch.st.size() * sizeof(WalkState), hipMemcpyDeviceToHost, s), "D2H") ||
        !hip_ok(hipStreamSynchronize(s), "sync") || !hip_ok(hipEventElapsedTime(&f, ev.e[0], ev.e[1]), "hipEventElapsedTime") ||
        !hip_ok(hipEventElapsedTime(&w, ev.e[1], ev.e[2]), "hipEventElapsedTime"))
        return PA_E_HIP;
    *refill_ms += f;
    *walk_ms += w;
    return 0;
}

}  // namespace

extern "C" int pa_affine_batch_align_tiled(pa_affine_batch* ab, uint32_t tile_cols, int32_t* cost_out, char** cigar_out, float* forward_ms,
                                           float* refill_ms, float* walk_ms) {
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_align_tiled: NULL batch");
    if (forward_ms) *forward_ms = 0;
    if (refill_ms) *refill_ms = 0;
    if (walk_ms) *walk_ms = 0;
    if (cigar_out)
        for (size_t p = 0; p < ab->np; ++p) cigar_out[p] = nullptr;
    if (!ab->trace) return fail(PA_E_ARG, "pa_affine_batch_align_tiled: the batch was created without trace");
    if (tile_cols != 0 && (tile_cols < kTileColsMin || tile_cols > kTileColsMax))
        return fail(PA_E_ARG, "pa_affine_batch_align_tiled: tile_cols = %u outside [%u, %u] (0 = the default, %u)", tile_cols, kTileColsMin, kTileColsMax,
                    kTileColsDefault);
    const uint32_t C = tile_cols ? tile_cols : kTileColsDefault;
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    for (size_t p = 0; p < ab->np; ++p)
        if (tiled_bytes_of(ab->n[p], ab->m[p], C) > budget)
            return fail(PA_E_ARG, "pa_affine_batch_align_tiled: pair %zu: %zu bytes of checkpoints, tile and ops exceed the budget of %zu bytes", p,
                        tiled_bytes_of(ab->n[p], ab->m[p], C), budget);
    hipStream_t s = 0;
    std::vector<std::string> cigars(ab->np);
    std::vector<int64_t> starts(ab->np, 0);
    ab->tiled = {};
    if (ab->chain.on) ab->chain.pairs = ab->chain.jobs = ab->chain.chunks = ab->chain.bnd_bytes_max = 0;
    float fwd_total = 0, refill_total = 0, walk_total = 0;
    std::vector<TileJob> jobs;
    std::vector<TileWave> waves;
    for (size_t c0 = 0, bytes; c0 < ab->np;) {
        const std::vector<uint32_t> ids = next_chunk(*ab, c0, budget, [&](uint32_t p) { return tiled_bytes_of(ab->n[p], ab->m[p], C); }, &bytes);
        ab->tiled.chunks += 1;
        ab->tiled.chunk_bytes_max = std::max(ab->tiled.chunk_bytes_max, (double)bytes);
        TiledChunk ch;
        float f = 0;
        if (const int rc = tiled_forward(*ab, ids, C, ch, s, &f)) return rc;
        fwd_total += f;
        Events ev;
        if (!ev.make()) return PA_E_HIP;
        for (;;) {  // ends: every round moves each unfinished pair into another tile, and tiled_jobs() bounds the tiles of a pair
            if (const int rc = tiled_jobs(*ab, C, ch, jobs, waves)) return rc;
            if (jobs.empty()) break;
            ab->tiled.rounds += 1;
            if (const int rc = tiled_round(*ab, ch, jobs, waves, ev, s, &refill_total, &walk_total)) return rc;
        }
        std::vector<uint8_t> ops(ch.ops_bytes);
        if (ch.ops_bytes && (!hip_ok(hipMemcpyAsync(ops.data(), ch.d_ops.ptr, ch.ops_bytes, hipMemcpyDeviceToHost, s), "D2H") ||
                             !hip_ok(hipStreamSynchronize(s), "sync")))
            return PA_E_HIP;
        for (size_t k = 0; k < ch.plan.pairs.size(); ++k) {
            cigars[ch.plan.pairs[k].out] = cigar_of(ops.data() + ch.ops_off[k], ch.st[k].nops);
            starts[ch.plan.pairs[k].out] = ch.st[k].i;
        }
        c0 += ids.size();
    }
    if (const int rc = costs_out(*ab, cost_out, s, &starts)) return rc;
    if (forward_ms) *forward_ms = fwd_total;
    if (refill_ms) *refill_ms = refill_total;
    if (walk_ms) *walk_ms = walk_total;
    return cigar_out ? give_cstrings(cigars, cigar_out) : 0;
}

extern "C" void pa_affine_batch_tiled_info(const pa_affine_batch* ab, double* chunks, double* rounds, double* tile_jobs, double* refill_cells,
                                           double* chunk_bytes_max) {
    if (chunks) *chunks = ab ? ab->tiled.chunks : 0;
    if (rounds) *rounds = ab ? ab->tiled.rounds : 0;
    if (tile_jobs) *tile_jobs = ab ? ab->tiled.tile_jobs : 0;
    if (refill_cells) *refill_cells = ab ? ab->tiled.refill_cells : 0;
    if (chunk_bytes_max) *chunk_bytes_max = ab ? ab->tiled.chunk_bytes_max : 0;
}

extern "C" int pa_affine_batch_set_chain(pa_affine_batch* ab, int on) {
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_set_chain: NULL batch");
    if (on != 0 && on != 1) return fail(PA_E_ARG, "pa_affine_batch_set_chain: on = %d is neither 0 nor 1", on);
    if (on)
        if (const int rc = chain_build(*ab, 0)) return rc;
    ab->chain.on = on != 0;
    return 0;
}

extern "C" int pa_affine_batch_set_free_ends(pa_affine_batch* ab, int free_start, int free_end) {
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_set_free_ends: NULL batch");
    if ((free_start != 0 && free_start != 1) || (free_end != 0 && free_end != 1))
        return fail(PA_E_ARG, "pa_affine_batch_set_free_ends: free_start = %d, free_end = %d: each is 0 or 1", free_start, free_end);
    if ((free_start || free_end) && !ab->d_end.reserve(std::max<size_t>(ab->np, 1) * 4)) return PA_E_HIP;
    ab->C.ends = (free_start ? kFreeStart : 0) | (free_end ? kFreeEnd : 0);
    ab->ends.valid = false;
    return 0;
}

extern "C" int pa_affine_batch_ends(const pa_affine_batch* ab, int64_t* start_out, int64_t* end_out) {
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_ends: NULL batch");
    if (!ab->ends.valid) return fail(PA_E_ARG, "pa_affine_batch_ends: no run, align or align_tiled has succeeded under the current setting");
    if (start_out && ab->np) std::memcpy(start_out, ab->ends.start.data(), ab->np * 8);
    if (end_out && ab->np) std::memcpy(end_out, ab->ends.end.data(), ab->np * 8);
    return 0;
}

// A cost-only pass of its own over the pairs that are asked for, in chunks whose rows fit the budget.  (It leaves costs and ends of its
// chunks in d_cost and d_end, which every other call reads only right after its own pass.)
extern "C" int pa_affine_batch_last_row(pa_affine_batch* ab, int32_t* out, const uint64_t* offsets) {
    if (!ab) return fail(PA_E_ARG, "pa_affine_batch_last_row: NULL batch");
    if (ab->np == 0) return 0;
    if (!out || !offsets) return fail(PA_E_ARG, "pa_affine_batch_last_row: NULL array");
    const size_t budget = trace_budget("PA_AFFINE_TRACE_BUDGET_MB");
    std::vector<uint32_t> want;
    for (const uint32_t p : ab->order)
        if (offsets[p] != UINT64_MAX) {
            if (((size_t)ab->n[p] + 1) * 4 > budget)
                return fail(PA_E_ARG, "pa_affine_batch_last_row: pair %u: %zu bytes of last row exceed the budget of %zu bytes", p, ((size_t)ab->n[p] + 1) * 4,
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
        Plan P;
        if (const int rc = make_plan(*ab, ids, P, nullptr, s)) return rc;
        rows.resize(words);
        if (!d_rows.reserve(words * 4) || !upload(d_off, off.data(), off.size() * 8, s)) return PA_E_HIP;
        const Ends E{ab->d_end.as<int32_t>(), d_rows.as<int32_t>(), d_off.as<uint64_t>()};
        if (!launch<false>(*ab, P.d_waves.as<Wave>(), P.waves.size(), P.d_pairs.as<Pair>(), s, &E) ||
            !hip_ok(hipMemcpyAsync(rows.data(), d_rows.ptr, words * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        for (const uint32_t p : ids) std::memcpy(out + offsets[p], rows.data() + off[p], ((size_t)ab->n[p] + 1) * 4);
        c0 = c1;
    }
    return 0;
}

extern "C" void pa_affine_batch_chain_info(const pa_affine_batch* ab, double* on, double* chain_pairs, double* chain_jobs, double* chunks,
                                           double* bnd_bytes_max) {
    if (on) *on = ab && ab->chain.on ? 1 : 0;
    if (chain_pairs) *chain_pairs = ab ? ab->chain.pairs : 0;
    if (chain_jobs) *chain_jobs = ab ? ab->chain.jobs : 0;
    if (chunks) *chunks = ab ? ab->chain.chunks : 0;
    if (bnd_bytes_max) *bnd_bytes_max = ab ? ab->chain.bnd_bytes_max : 0;
}

extern "C" void pa_affine_batch_info(const pa_affine_batch* ab, double* waves, double* packed_pairs, double* strip_pairs, double* lane_use,
                                     double* trace_chunks) {
    if (waves) *waves = ab ? (double)ab->fwd.waves.size() : 0;
    if (packed_pairs) *packed_pairs = ab ? (double)ab->fwd.packed : 0;
    if (strip_pairs) *strip_pairs = ab ? (double)ab->fwd.strip : 0;
    if (lane_use) *lane_use = ab && ab->fwd.slots > 0 ? ab->fwd.lanes / ab->fwd.slots : 0;
    if (trace_chunks) *trace_chunks = ab ? ab->trace_chunks : 0;
}

extern "C" void pa_affine_batch_destroy(pa_affine_batch* ab) {
    if (!ab) return;
    (void)hipDeviceSynchronize();
    dt_release(ab->dt);
    delete ab;
}
