// apa2_jobs_unit.hip -- how the per-pair jobs of the batched A*PA2 modes are built at creation (pa_batch_create_params): offsets, host-built
// heuristic tables, buffers, PairJob / FullJob, the build kernel's scratch and jobs, the start order.  One entry, apa2_make_jobs; the
// builders below are lists of file-static phases.  No kernels: the launches go through apa2_units.hpp.
#include "pa_batch.hpp"
#include "engine_capi.hpp"

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

// Words per slot of a pair's block-column store.  Measured on the CPU-kernel engine (round 4): `simple` on 100 kbp at 5 % ends with bands of
// 133 words within 69 words of the main diagonal, 10 kbp at 15 % with 37 within 20; `full` (GCSH) on 100 kbp at 5 % with 12 within 7.
// The windows below hold those with room to spare; what does not fit (15 % on 100 kbp: 260 words) is aligned again with full columns.
size_t pa::window_words(size_t n, size_t m, bool gcsh, int override_) {
    const size_t wtot = std::max<size_t>((m + 63) / 64, 1);
    static const int env = getenv("PA_APA2_WINDOW") ? atoi(getenv("PA_APA2_WINDOW")) : -1;
    const int o = override_ >= 0 ? override_ : env;
    if (o == 0) return wtot;
    size_t W = o > 0 ? (size_t)o : (gcsh ? 64 : ((2 * ((std::max(n, m) + 1249) / 1250) + 32 + 7) & ~size_t(7)));
    return std::min(W, wtot);
}

// Host threads for per-pair host work of a batch (the matches of GCSH, the SH tables): as many as the process may run on.
unsigned pa::host_threads() {
    static const unsigned n = [] {
        if (const char* e = getenv("PA_HOST_THREADS")) return (unsigned)std::max(1, atoi(e));
        unsigned c = 0;
#if defined(__linux__)
        cpu_set_t set;
        CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof set, &set) == 0) c = (unsigned)CPU_COUNT(&set);
#endif
        if (c == 0) c = std::thread::hardware_concurrency();
        return std::max(1u, std::min(c, 64u));
    }();
    return n;
}
template <class F>
static void parallel_pairs(size_t P, F&& f) {
    const unsigned nt = (unsigned)std::min<size_t>(host_threads(), std::max<size_t>(P, 1));
    if (nt <= 1) {
        for (size_t i = 0; i < P; ++i) f(i);
        return;
    }
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&] {
            for (size_t i = next.fetch_add(1); i < P; i = next.fetch_add(1)) f(i);
        });
    for (auto& t : th) t.join();
}

// The start order of the batched band search: the most expensive pairs first (sketch_unit.hip has the why).  Expected work of a pair:
// its length times the band its final pass needs, band ~ estimated cost = e (n + m) / 2 with e from the sketch ((1 - e)^16 = found / 64).
// PA_APA2_ORDER_INPUT keeps the caller's order, PA_APA2_ORDER_LENGTH the order of the lengths (round 4) -- experiments and tests.
static bool astar_start_order(pa_batch* p, std::vector<int32_t>& order) {
    const size_t P = p->pairs;
    order.resize(P);
    for (size_t i = 0; i < P; ++i) order[i] = (int32_t)i;
    if (getenv("PA_APA2_ORDER_INPUT") || P < 2) return true;
    PhaseClock clock("pa_batch_create");
    static_assert(sizeof(apa2::SketchDesc) == sizeof(PairDesc), "the sketch reads the batch's pair descriptors");
    std::vector<uint8_t> found(P, 64);
    const bool sketch = !getenv("PA_APA2_ORDER_LENGTH");
    if (sketch) {
        if (!p->d_sketch.alloc(P) ||
            !hip_ok(apa2::launch_sketch_kernel(p->stream, p->d_a.as<uint8_t>(), p->d_b.as<uint8_t>(), (const apa2::SketchDesc*)p->d_desc.ptr, (int)P, p->d_sketch.as<uint8_t>()),
                    "sketch_kernel launch") ||
            !hip_ok(hipMemcpyAsync(found.data(), p->d_sketch.ptr, P, hipMemcpyDeviceToHost, p->stream), "D2H sketch") || !hip_ok(hipStreamSynchronize(p->stream), "sync"))
            return false;
    }
    const double sketch_ms = clock.lap();
    // e from found / 64 = (1 - e)^16, by table (nothing found: as if half a sample had been)
    double e_of[65];
    for (int f = 0; f <= 64; ++f) e_of[f] = 1.0 - std::pow(std::max(0.5, (double)f) / 64.0, 1.0 / 16.0);
    // descending by the expected work, ties in the caller's order: one sort of 64-bit words (float bits of a positive key order like integers)
    std::vector<uint64_t> keyed(P);
    for (size_t i = 0; i < P; ++i) {
        const float len = (float)(p->n[i] + p->m[i]);
        const float key = sketch ? len * ((float)e_of[std::min<int>(found[i], 64)] * len * 0.5f + 128.0f) : len;
        uint32_t bits;
        std::memcpy(&bits, &key, 4);
        keyed[i] = ((uint64_t)bits << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
    }
    std::sort(keyed.begin(), keyed.end(), std::greater<uint64_t>());
    for (size_t i = 0; i < P; ++i) order[i] = (int32_t)(0xFFFFFFFFu - (uint32_t)(keyed[i] & 0xFFFFFFFFu));
    if (align_profile()) std::fprintf(stderr, "[%s]   start order: sketch %.3f ms, sort %.3f ms\n", clock.tag, sketch_ms, clock.lap());
    return true;
}

// ---- layouts: pure functions of the pairs' lengths and the parameter set (no plan, no device) -----------------------------

// Seeds of GCSH in a sequence of n characters: every hk-th k-mer that fits.
static size_t seeds_of(size_t n, int32_t hk) { return n >= (size_t)hk ? (n - hk) / hk + 1 : 0; }

// Where pair i's slice of every per-pair buffer starts, and the totals: summed once per batch, read by both builders.
struct JobOffsets {
    std::vector<size_t> rec_off, sh_off;  // block records (d_rec, d_jh), entries of the SH table (d_sh)
    size_t tr = 0, tsh = 0;
    // the full family on top: columns of the h row (d_hrow), seeds (d_win, d_win0), matches (d_mi .. d_cell; [pairs] = the total)
    std::vector<size_t> col_off, seed_off, match_off;
    size_t tn = 0, tseeds = 0, tm = 0;
    // ... and when the GPU finds the matches: candidate slots and hash-table entries of the build kernel per pair
    std::vector<size_t> cap, tsz;
    size_t ttab = 0;
};
static JobOffsets sum_offsets(const std::vector<size_t>& n, bool sh, bool full, bool gcsh, bool device_build, int32_t hk) {
    const size_t P = n.size();
    JobOffsets o;
    o.rec_off.resize(P);
    o.sh_off.resize(P);
    if (full) {
        o.col_off.resize(P);
        o.seed_off.resize(P);
        o.match_off.assign(P + 1, 0);  // (matches from host threads: place_host_matches, once they are found)
        o.cap.assign(P, 0);
        o.tsz.assign(P, 0);
    }
    for (size_t i = 0; i < P; ++i) {
        o.rec_off[i] = o.tr;
        o.tr += (n[i] + 255) / 256 + 2;
        o.sh_off[i] = o.tsh;
        if (sh) o.tsh += n[i] + 1;
        if (!full) continue;
        const size_t ns = gcsh ? seeds_of(n[i], hk) : 0;
        o.col_off[i] = o.tn;
        o.tn += (n[i] + 63) & ~size_t(63);
        o.seed_off[i] = o.tseeds;
        o.tseeds += ns;
        o.match_off[i] = o.tm;
        if (!device_build) continue;
        // room for the candidates of a pair: every seed once and half of them again, plus 2048 (a pair that needs more -- a
        // repeat-rich sequence -- is flagged by the kernel and goes to the host engine)
        o.cap[i] = ns + ns / 2 + 2048;
        o.tsz[i] = 64;
        while (o.tsz[i] < 2 * ns + 1) o.tsz[i] *= 2;
        o.ttab += o.tsz[i];
        o.tm += o.cap[i];
    }
    if (full) o.match_off[P] = o.tm;
    return o;
}

// Scratch of the build kernel, one slice per pair: u32 keys / next_same / cnt / fill per seed, the table, four ints and two bytes per
// candidate slot.  One walk gives every array's place and the totals: the allocation and the GcshBuildJob pointers both come from it.
struct BuildSlice {
    size_t keys, next_same, cnt, fill, slot, tmp_s, tmp_j, gpos, cj;  // in ints from the start of the scratch
    size_t flag, keptg;                                               // in bytes from the end of the ints
};
struct BuildLayout {
    std::vector<BuildSlice> at;
    size_t words = 0, tail_bytes = 0;
    size_t bytes() const { return words * 4 + tail_bytes + 64; }
};
static BuildLayout build_scratch_layout(const std::vector<size_t>& n, const JobOffsets& o, int32_t hk) {
    BuildLayout l;
    l.at.resize(n.size());
    auto take = [](size_t& total, size_t count) {
        const size_t at = total;
        total += count;
        return at;
    };
    for (size_t i = 0; i < n.size(); ++i) {
        const size_t ns = seeds_of(n[i], hk);
        BuildSlice& s = l.at[i];
        s.keys = take(l.words, ns);
        s.next_same = take(l.words, ns);
        s.cnt = take(l.words, ns + 1);
        s.fill = take(l.words, ns);
        s.slot = take(l.words, o.tsz[i]);
        s.tmp_s = take(l.words, o.cap[i]);
        s.tmp_j = take(l.words, o.cap[i]);
        s.gpos = take(l.words, o.cap[i]);
        s.cj = take(l.words, o.cap[i]);
        s.flag = take(l.tail_bytes, o.cap[i]);
        s.keptg = take(l.tail_bytes, o.cap[i]);
    }
    return l;
}

// ---- what the two builders share --------------------------------------------------------------------------------------

// The search parameters of apa2_kernel.hpp from the engine's; the full family reads the heuristic kind from them too.
static void search_params(const engine::AstarPa2Params& ap, pa_batch* p) {
    p->sp.heur = ap.heuristic == engine::HeuristicKind::Gap ? sweep::kHeurGap : (ap.heuristic == engine::HeuristicKind::SH ? sweep::kHeurSH : sweep::kHeurNone);
    p->sp.sparse_h = ap.sparse_h ? 1 : 0;
    p->sp.doubling = ap.doubling == engine::DoublingKind::LinearSearch ? apa2::kDoublingLinear : apa2::kDoublingBand;
    p->sp.start = (int32_t)ap.start;
    p->sp.factor = ap.factor;
    p->sp.delta = (int32_t)ap.delta;
}

// SeedHeuristicH (pa-heuristic sh.rs:47-106): the per-column table of every pair, built on host threads (a pair with an empty sequence
// is left to the host engine: its entries stay zero).
static std::vector<int32_t> sh_tables(const pa_batch* p, const uint8_t* const* a, const uint8_t* const* b, const engine::AstarPa2Params& ap, const JobOffsets& off) {
    std::vector<int32_t> sh(off.tsh);
    if (off.tsh)
        parallel_pairs(p->pairs, [&](size_t i) {
            const engine::I n = (engine::I)p->n[i], m = (engine::I)p->m[i];
            if (n == 0 || m == 0) return;
            engine::SeedHeuristicH h(a[i], n, b[i], m, ap.heuristic_k, (int)ap.heuristic_p);
            std::copy(h.h_by_i.begin(), h.h_by_i.end(), sh.begin() + (long)off.sh_off[i]);
        });
    return sh;
}

// The fields PairJob and FullJob share.
template <class Job>
static void fill_common(Job& j, const pa_batch* p, size_t i, const JobOffsets& off) {
    j.a_codes = p->d_codes.as<uint32_t>() + p->code_off[i];
    j.b_prof = p->d_prof.as<uint32_t>() + p->prof_off[i] * 4;
    j.rec = p->d_rec.as<sweep::BlockRec>() + off.rec_off[i];
    j.col = p->d_ckpt.as<uint32_t>() + p->ckpt_off[i];
    j.col_stride = (int64_t)p->win_words[i];
    j.slot_ratio = p->slot_ratio[i];
    j.sh_h = p->sp.heur == sweep::kHeurSH ? p->d_sh.as<int32_t>() + off.sh_off[i] : nullptr;
    j.gran = p->d_scratch_gran.as<uint64_t>() + i * 16;
    j.sum = p->d_sums.as<int32_t>() + i;
    j.result = p->d_results.as<apa2::PairResult>() + i;
    j.n = (int32_t)p->n[i];
    j.m = (int32_t)p->m[i];
}

// The most expensive pairs first (astar_start_order); then the pairs' jobs and the order go to the device.
static bool upload_jobs_and_order(pa_batch* p, DeviceBuf& dst, const void* jobs, size_t bytes) {
    if (!astar_start_order(p, p->order_host)) return false;
    return !p->pairs || (hip_ok(hipMemcpy(dst.ptr, jobs, bytes, hipMemcpyHostToDevice), "H2D pair jobs") &&
                         hip_ok(hipMemcpy(p->d_order.ptr, p->order_host.data(), p->pairs * 4, hipMemcpyHostToDevice), "H2D order"));
}

// ---- the `simple` family (apa2_kernel.hpp) ------------------------------------------------------------------------------

// The per-pair descriptors of the A*PA2 mode; completes the trace jobs (banded blocks, statistics).
static bool astar_jobs(pa_batch* p, const uint8_t* const* a, const uint8_t* const* b, std::vector<TraceJob>& tjobs) {
    const engine::AstarPa2Params ap = engine::params_from_c(p->aparams_c);
    const size_t P = p->pairs;
    search_params(ap, p);
    const JobOffsets off = sum_offsets(p->n, p->sp.heur == sweep::kHeurSH, false, false, false, 1);
    if (!p->d_rec.alloc(std::max<size_t>(off.tr, 1) * sizeof(sweep::BlockRec)) || !p->d_results.alloc(std::max<size_t>(P, 1) * sizeof(apa2::PairResult)) ||
        !p->d_pjobs.alloc(std::max<size_t>(P, 1) * sizeof(apa2::PairJob)) || !p->d_order.alloc(std::max<size_t>(P, 1) * 4) ||
        !p->d_tstats.alloc(std::max<size_t>(P, 1) * 32) || !p->d_sh.alloc(std::max<size_t>(off.tsh, 1) * 4))
        return false;
    const std::vector<int32_t> sh = sh_tables(p, a, b, ap, off);
    if (off.tsh && !hip_ok(hipMemcpy(p->d_sh.ptr, sh.data(), off.tsh * 4, hipMemcpyHostToDevice), "H2D sh")) return false;
    std::vector<apa2::PairJob> pj(P);
    for (size_t i = 0; i < P; ++i) {
        fill_common(pj[i], p, i, off);
        pj[i].pad0 = 0;
        fill_trace_job(tjobs, p, i, pj[i].rec, pj[i].result);
    }
    return upload_jobs_and_order(p, p->d_pjobs, pj.data(), P * sizeof(apa2::PairJob));
}

// ---- the whole family (apa2_full_kernel.hpp) ----------------------------------------------------------------------------

// What the phases of astar_full_jobs share.
struct FullRun {
    pa_batch* p;
    const uint8_t* const* a;
    const uint8_t* const* b;
    std::vector<TraceJob>& tjobs;
    const engine::AstarPa2Params ap = engine::params_from_c(p->aparams_c);
    const bool gcsh = ap.heuristic == engine::HeuristicKind::GCSH, sh = ap.heuristic == engine::HeuristicKind::SH;
    const int32_t hk = ap.heuristic_k < 1 ? 1 : ap.heuristic_k;
    JobOffsets off;
    // from host threads: the SH table, or (GCSH, unless the GPU finds them) every pair's matches and the seeds' windows
    std::vector<int32_t> shv;
    std::vector<std::vector<int32_t>> pmi, pmj;
    std::vector<apa2::GcshSeedWindow> win;
    PhaseClock clock{"pa_batch_create"};  // diagnostics: where the creation time goes
};

// The parameters of both kernels' searches, who finds the matches, every pair's offsets.
// The matches of GCSH are found on the GPU, once, at the end of the creation (gcsh_build_kernel.hpp), when the look-ahead of local
// pruning fits its LDS arrays; PA_GCSH_HOST_BUILD=1 finds them on host threads at creation instead (tests compare the two).
static void size_full_layout(FullRun& r) {
    pa_batch* p = r.p;
    const engine::AstarPa2Params& ap = r.ap;
    search_params(ap, p);
    p->fsp.sparse_h = ap.sparse_h ? 1 : 0;
    p->fsp.prune = ap.prune ? 1 : 0;
    p->fsp.incremental = ap.front.incremental_doubling ? 1 : 0;
    p->fsp.doubling = ap.doubling == engine::DoublingKind::LinearSearch ? 2 : 1;
    p->fsp.start = (int32_t)ap.start;
    p->fsp.factor = ap.factor;
    p->fsp.delta = (int32_t)ap.delta;
    static const bool host_build_env = getenv("PA_GCSH_HOST_BUILD") != nullptr && getenv("PA_GCSH_HOST_BUILD")[0] != '0';
    p->device_build = r.gcsh && !host_build_env && ap.heuristic_p >= 0 && ap.heuristic_p <= apa2::kBuildMaxP && r.hk <= 31;
    r.off = sum_offsets(p->n, r.sh, true, r.gcsh, p->device_build, r.hk);
}

// The matches of GCSH (seeds, exact k-mer matches in the reference's push order, the transform filter, local pruning p: csrc/gcsh.hpp)
// of every pair, and where each pair's lie in the concatenation.
static void host_matches(FullRun& r) {
    const pa_batch* p = r.p;
    const size_t P = p->pairs;
    r.pmi.resize(P);
    r.pmj.resize(P);
    r.win.resize(r.off.tseeds);
    parallel_pairs(P, [&](size_t i) {
        const engine::I n = (engine::I)p->n[i], m = (engine::I)p->m[i];
        if (n == 0 || m == 0) return;
        engine::GcshHeuristic gh(r.a[i], n, r.b[i], m, r.ap.heuristic_k, (int)r.ap.heuristic_p, r.ap.prune, false);
        r.pmi[i].reserve(gh.by_start.size());
        r.pmj[i].reserve(gh.by_start.size());
        for (const auto& mt : gh.by_start) {
            r.pmi[i].push_back(mt.i);
            r.pmj[i].push_back(mt.j);
        }
        for (size_t s = 0; s < gh.active_range.size(); ++s)
            r.win[r.off.seed_off[i] + s] = apa2::GcshSeedWindow{(int32_t)gh.active_range[s].b0, (int32_t)gh.active_range[s].b1, -1, 0};
    });
    for (size_t i = 0; i < P; ++i) {
        r.off.match_off[i] = r.off.tm;
        r.off.tm += r.pmi[i].size();
    }
    r.off.match_off[P] = r.off.tm;
}

// Host threads: the matches (GCSH, unless the GPU finds them) / the per-column table (SH) of every pair.
static void host_heuristic_tables(FullRun& r) {
    pa_batch* p = r.p;
    const auto t0 = std::chrono::steady_clock::now();
    if (r.sh) r.shv = sh_tables(p, r.a, r.b, r.ap, r.off);
    if (r.gcsh && !p->device_build) host_matches(r);
    p->full_matches = r.off.tm;
    p->full_seeds = r.off.tseeds;
    p->full_build_ms = p->device_build ? 0.0 : std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    r.clock.mark("  full: host tables / sizes");
}

static bool alloc_full_buffers(FullRun& r) {
    pa_batch* p = r.p;
    const size_t P1 = std::max<size_t>(p->pairs, 1), tr = r.off.tr, tsh = r.off.tsh, tn = r.off.tn, tm = r.off.tm, tseeds = r.off.tseeds;
    if (!p->d_rec.alloc(std::max<size_t>(tr, 1) * sizeof(sweep::BlockRec)) || !p->d_jh.alloc(std::max<size_t>(tr, 1) * 4) ||
        !p->d_results.alloc(P1 * sizeof(apa2::PairResult)) || !p->d_fjobs.alloc(P1 * sizeof(apa2::FullJob)) ||
        !p->d_order.alloc(P1 * 4) || !p->d_tstats.alloc(P1 * 32) || !p->d_sh.alloc(std::max<size_t>(tsh, 1) * 4) ||
        !p->d_hrow.alloc(std::max<size_t>(tn, 64)) || !p->d_mi.alloc(std::max<size_t>(tm, 1) * 4) || !p->d_mj.alloc(std::max<size_t>(tm, 1) * 4) ||
        !p->d_active.alloc(std::max<size_t>(tm, 64)) || !p->d_win.alloc(std::max<size_t>(tseeds, 1) * sizeof(apa2::GcshSeedWindow)) ||
        !p->d_win0.alloc(std::max<size_t>(tseeds, 1) * sizeof(apa2::GcshSeedWindow)) ||
        !p->d_lrec.alloc((tm + 2 * P1) * sizeof(apa2::GcshCell)) || !p->d_cell.alloc(std::max<size_t>(tm, 1) * sizeof(apa2::GcshCell)) ||
        !p->d_probe.alloc(128 + 8 * P1))  // (16 counters, then per pair: HW_ID / XCC_ID and the ticks of its band search; PA_APA2_PROBE_STATS)
        return false;
    r.clock.mark("  full: device buffers");
    return true;
}

// What the host threads built.  (The GPU's builder writes d_mi / d_mj / d_win0 itself: nothing to upload then.)
static bool upload_host_tables(FullRun& r) {
    pa_batch* p = r.p;
    const size_t P = p->pairs, tsh = r.off.tsh, tm = r.off.tm, tseeds = r.off.tseeds;
    if (tsh && !hip_ok(hipMemcpy(p->d_sh.ptr, r.shv.data(), tsh * 4, hipMemcpyHostToDevice), "H2D sh")) return false;
    if (p->device_build) return true;
    if (tm) {
        std::vector<int32_t> mi(tm), mj(tm);
        for (size_t i = 0; i < P; ++i) {
            std::copy(r.pmi[i].begin(), r.pmi[i].end(), mi.begin() + (long)r.off.match_off[i]);
            std::copy(r.pmj[i].begin(), r.pmj[i].end(), mj.begin() + (long)r.off.match_off[i]);
        }
        if (!hip_ok(hipMemcpy(p->d_mi.ptr, mi.data(), tm * 4, hipMemcpyHostToDevice), "H2D matches") ||
            !hip_ok(hipMemcpy(p->d_mj.ptr, mj.data(), tm * 4, hipMemcpyHostToDevice), "H2D matches"))
            return false;
    }
    return !tseeds || hip_ok(hipMemcpy(p->d_win0.ptr, r.win.data(), tseeds * sizeof(apa2::GcshSeedWindow), hipMemcpyHostToDevice), "H2D seed windows");
}

// The build kernel's scratch, status words, ticket and per-pair jobs (only when the GPU finds the matches).
static bool make_build_jobs(FullRun& r) {
    pa_batch* p = r.p;
    const size_t P = p->pairs;
    if (!p->device_build) return true;
    const BuildLayout lay = build_scratch_layout(p->n, r.off, r.hk);
    if (!p->d_bscratch.alloc(lay.bytes()) || !p->d_bjobs.alloc(std::max<size_t>(P, 1) * sizeof(apa2::GcshBuildJob)) || !p->d_bstatus.alloc(std::max<size_t>(P, 1) * 4) ||
        !p->d_bticket.alloc(64) || !hip_ok(hipEventCreate(&p->evB0), "event") || !hip_ok(hipEventCreate(&p->evB1), "event"))
        return false;
    r.clock.mark("  full:   build: buffers");
    int32_t* w32 = p->d_bscratch.as<int32_t>();
    uint8_t* w8 = (uint8_t*)(w32 + lay.words);
    std::vector<apa2::GcshBuildJob> bj(P);
    for (size_t i = 0; i < P; ++i) {
        const BuildSlice& s = lay.at[i];
        apa2::GcshBuildJob& x = bj[i];
        std::memset(&x, 0, sizeof x);
        x.a = p->d_a.as<uint8_t>() + p->a_off[i];
        x.b = p->d_b.as<uint8_t>() + p->b_off[i];
        x.keys = (uint32_t*)(w32 + s.keys);
        x.next_same = w32 + s.next_same;
        x.cnt = w32 + s.cnt;
        x.fill = w32 + s.fill;
        x.slot = w32 + s.slot;
        x.tmp_s = w32 + s.tmp_s;
        x.tmp_j = w32 + s.tmp_j;
        x.gpos = w32 + s.gpos;
        x.cj = w32 + s.cj;
        x.flag = w8 + s.flag;
        x.keptg = w8 + s.keptg;
        x.mi = p->d_mi.as<int32_t>() + r.off.match_off[i];
        x.mj = p->d_mj.as<int32_t>() + r.off.match_off[i];
        x.win0 = p->d_win0.as<apa2::GcshSeedWindow>() + r.off.seed_off[i];
        x.nmatch_out = &p->d_fjobs.as<apa2::FullJob>()[i].g.nmatch;
        x.status = p->d_bstatus.as<uint32_t>() + i;
        x.n = (int32_t)p->n[i];
        x.m = (int32_t)p->m[i];
        x.k = r.hk;
        x.p = (int32_t)r.ap.heuristic_p;
        x.nseeds = (int32_t)seeds_of(p->n[i], r.hk);
        x.tsize = (int32_t)r.off.tsz[i];
        x.cap = (int32_t)r.off.cap[i];
    }
    r.clock.mark("  full:   build: descriptors");
    if (P && !hip_ok(hipMemcpy(p->d_bjobs.ptr, bj.data(), P * sizeof(apa2::GcshBuildJob), hipMemcpyHostToDevice), "H2D build jobs")) return false;
    r.clock.mark("  full:   build: H2D");
    return true;
}

static void make_full_jobs(FullRun& r, std::vector<apa2::FullJob>& fj) {
    const pa_batch* p = r.p;
    const JobOffsets& off = r.off;
    for (size_t i = 0; i < p->pairs; ++i) {
        apa2::FullJob& j = fj[i];
        std::memset(&j, 0, sizeof j);
        fill_common(j, p, i, off);
        j.jh = p->d_jh.as<int32_t>() + off.rec_off[i];
        j.hrow = p->d_hrow.as<uint8_t>() + off.col_off[i];
        j.heur = (int32_t)r.ap.heuristic;
        if (r.gcsh) {
            apa2::GcshDev& g = j.g;
            g.mi = p->d_mi.as<int32_t>() + off.match_off[i];
            g.mj = p->d_mj.as<int32_t>() + off.match_off[i];
            g.active = p->d_active.as<uint8_t>() + off.match_off[i];
            g.win = p->d_win.as<apa2::GcshSeedWindow>() + off.seed_off[i];
            g.lrec = p->d_lrec.as<apa2::GcshCell>() + off.match_off[i] + 2 * i;
            g.cell = p->d_cell.as<apa2::GcshCell>() + off.match_off[i];
            g.nmatch = (int32_t)(off.match_off[i + 1] - off.match_off[i]);
            g.nlayers = 1;
            g.n = j.n;
            g.m = j.m;
            g.k = r.hk;
            g.nseeds = (int32_t)seeds_of(p->n[i], r.hk);
            g.prune = r.ap.prune ? 1 : 0;
        }
        fill_trace_job(r.tjobs, p, i, j.rec, j.result);
    }
}

// The matches of GCSH are part of the batch like the sequences they are derived from: found here, once, by the GPU (one wavefront
// per pair, 12.8 KB of LDS each: twelve to a CU), on the batch's stream -- the first alignment call queues behind it.
static bool launch_match_build(FullRun& r) {
    pa_batch* p = r.p;
    const size_t P = p->pairs;
    if (!p->device_build || !P) return true;
    const int cus = device_cus();
    static const int per_cu = getenv("PA_BUILD_WAVES_PER_CU") ? std::max(1, atoi(getenv("PA_BUILD_WAVES_PER_CU"))) : 12;
    const int grid = (int)std::min<size_t>(P, (size_t)cus * (size_t)per_cu);
    return hip_ok(hipMemsetAsync(p->d_bticket.ptr, 0, 64, p->stream), "memset") && hip_ok(hipEventRecord(p->evB0, p->stream), "event") &&
           hip_ok(apa2::launch_gcsh_build_kernel(grid, p->stream, p->d_bjobs.as<apa2::GcshBuildJob>(), (int)P, p->d_bticket.as<uint32_t>()), "gcsh_build_kernel launch") &&
           hip_ok(hipEventRecord(p->evB1, p->stream), "event");
}

// The per-pair descriptors of the whole-family mode (apa2_full_kernel.hpp); completes the trace jobs like astar_jobs.  The matches of
// GCSH are found by the GPU's build kernel or on host threads; the contours are derived on the device either way.
static bool astar_full_jobs(pa_batch* p, const uint8_t* const* a, const uint8_t* const* b, std::vector<TraceJob>& tjobs) {
    FullRun r{p, a, b, tjobs};
    size_full_layout(r);
    host_heuristic_tables(r);
    if (!alloc_full_buffers(r) || !upload_host_tables(r) || !make_build_jobs(r)) return false;
    r.clock.mark("  full: build scratch + jobs");
    std::vector<apa2::FullJob> fj(p->pairs);
    make_full_jobs(r, fj);
    if (!upload_jobs_and_order(p, p->d_fjobs, fj.data(), p->pairs * sizeof(apa2::FullJob))) return false;
    r.clock.mark("  full: pair jobs + order");
    return launch_match_build(r);
}

bool apa2_make_jobs(pa_batch* p, const uint8_t* const* a, const uint8_t* const* b, std::vector<TraceJob>& tjobs) {
    return p->astar_full ? astar_full_jobs(p, a, b, tjobs) : astar_jobs(p, a, b, tjobs);
}
