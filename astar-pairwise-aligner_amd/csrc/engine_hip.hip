// engine_hip.hip -- pa_align, the pa_bp_ctx_* handles and what the astarpa-c symbols run through: the A*PA2 block engine
// (engine.hpp) over HipBackend (hip_backend.hpp), the device-side sweep (sweep_hip.hpp) and the call combiner (combine_unit.hip).
// Every rectangle and sweep kernel these launch is instantiated in this translation unit.
#include <atomic>
#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "engine_capi.hpp"
#include "hip_backend.hpp"
#include "pa_hip_internal.hpp"
#include "sweep_hip.hpp"

namespace pa {

// More hardware queues for the pipelined passes.  NOT done behind the application's back when the library is loaded (a library that
// edits the process environment at dlopen surprises every other HIP user in the process and races with their getenv): the
// application calls this once, before anything starts the HIP runtime, or exports the variable itself.  Returns 1 if it set the
// variable, 0 if it was set already (left alone).
extern "C" int pa_runtime_hints(void) {
    if (std::getenv("GPU_MAX_HW_QUEUES")) return 0;
    return setenv("GPU_MAX_HW_QUEUES", "16", 0) == 0 ? 1 : 0;
}

// pa_align and the drop-in symbols keep their device buffers, pinned staging and streams in per-thread pools that only grow (one
// 10 Mbp call leaves gigabytes behind): this returns the calling thread's pools to the driver.  The next call builds them again.
extern "C" void pa_release_pools(void) {
    (void)hipDeviceSynchronize();
    sweep_pool_slot().reset();
    pooled_backend_slot().reset();
    release_alloc_cache();  // (after the pools: their buffers land in the cache first)
}

// The engine's bookkeeping without any kernel work (used where the numbers come from a fused GPU pass).
struct StatsOnlyBackend {
    const uint8_t* a_;
    size_t n_;
    const uint8_t* b_;
    size_t m_;
    I n() const { return (I)n_; }
    I m() const { return (I)m_; }
    const uint8_t* a() const { return a_; }
    const uint8_t* b() const { return b_; }
    void enable_h_row() {}
    Cost compute(I, I, size_t, size_t, V*, HMode, const BlockParams&) { return 0; }
    void fill(I, I, size_t, size_t, V*, V*, int8_t*, const BlockParams&) {}
    std::vector<int8_t> debug_read_h(I, I) { return {}; }
    void debug_write_h(I, I, const std::vector<int8_t>&) {}
};

static std::atomic<int> g_reference_cost_only{0};
static bool reference_cost_only_requested() {
    if (g_reference_cost_only.load(std::memory_order_relaxed)) return true;
    const char* e = std::getenv("PA_COST_ONLY_MODE");
    return e && std::strcmp(e, "reference") == 0;
}
extern "C" void pa_set_reference_cost_only(int on) { g_reference_cost_only.store(on ? 1 : 0, std::memory_order_relaxed); }

// ---- the routes of align_hip ----------------------------------------------------------------------------------------------------

// AstarPa2Params::nw().make_aligner(false): the whole matrix, cost only (blocks.rs:252-277: one block updated in
// place, 256 columns per operator call).  The values do not depend on the schedule, so the cost comes from ONE
// launch of chained strips (pa_batch of one pair) instead of |a|/256 launches; the statistics come from the host
// engine walked over a backend that computes nothing (they depend on the lengths only).
static int align_full_matrix_cost(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, const engine::AstarPa2Params& p, bool want_stats,
                                  engine::AlignResult& r) {
    const uint8_t* aa[1] = {a};
    const uint8_t* bb[1] = {b};
    const size_t al[1] = {a_len}, bl[1] = {b_len};
    pa_batch* bt = pa_batch_create(aa, al, bb, bl, 1);
    if (!bt) return PA_E_HIP;
    int32_t c = 0;
    const int rc = pa_batch_run(bt, &c, nullptr);
    pa_batch_destroy(bt);
    if (rc != 0) return rc;
    if (want_stats) {
        StatsOnlyBackend sb{a, a_len, b, b_len};
        r = engine::cost_or_align(p, sb, false, false);
    }
    r.cost = c;
    r.has_cigar = false;
    return 0;
}

// Domain::Astar with a closed-form / per-column heuristic and the sparse, non-incremental block engine (the `simple`
// preset and its relatives): every align_for_bounded_dist pass is ONE persistent launch with the band logic in the kernel
// (sweep_wave.hpp).  False: the kernel handed a pass back (SweepFallback), the pair is redone by the host-driven engine.
static bool align_sweep(const engine::AstarPa2Params& p, HipBackend& be, bool trace, engine::AlignResult& r) {
    try {
        HipSweepLauncher launcher(be, sweep_pool());
        launcher.heur_kind = p.heuristic == engine::HeuristicKind::Gap ? sweep::kHeurGap
                             : p.heuristic == engine::HeuristicKind::SH ? sweep::kHeurSH : sweep::kHeurNone;
        sweep::SweepAligner<HipBackend, HipSweepLauncher> al(p, be, launcher, trace);
        r = al.align();
        return true;
    } catch (const sweep::SweepFallback& e) {
        if (std::getenv("PA_SWEEP_TIMING")) std::fprintf(stderr, "sweep fallback: %s (%d)\n", e.what(), e.reason);
        return false;
    }
}

// The host-driven engine over the HIP operators: one launch per block, band logic on the host.
// traced_for_cost -- cost only, for the parameters the sweep serves: the sweep computes the band of the TRACED mode (its answer is the
// distance itself, its statistics those of the traced band; include/pa_astarpa2.h).  A pair it hands back gets the same: the host-driven
// engine in traced mode with the CIGAR dropped -- not the reference's cost-only single-block mode (blocks.rs:252-277), whose
// fixed range is the union over all columns (a triangle of the matrix) and which this restatement has seen end on an upper
// bound.  PA_ENGINE_NO_SWEEP (tests, diagnostics) still runs that mode as restated.
static void align_host_engine(const engine::AstarPa2Params& p, HipBackend& be, bool trace, bool traced_for_cost, bool self_check,
                              engine::AlignResult& r) {
    r = engine::cost_or_align(p, be, trace || traced_for_cost, self_check);
    if (traced_for_cost) {
        r.has_cigar = false;
        r.cigar = engine::Cigar();
        r.stats.trace_stats = engine::TraceStats();
    }
}

// Shared by pa_align and the astarpa-c symbols.  Returns 0 or a PA_E_* code.
int align_hip(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, const pa_astarpa2_params& params,
              bool trace, bool self_check, int32_t* cost_out, std::string* cigar_out, pa_astarpa2_stats* stats_out) {
    if (!engine::params_valid(params)) {
        set_error("invalid A*PA2 parameters");
        return PA_E_ARG;
    }
    if (a_len > (size_t)(1u << 30) || b_len > (size_t)(1u << 30)) {
        set_error("sequence too long for i32 coordinates");
        return PA_E_ARG;
    }
    const engine::AstarPa2Params p = engine::params_from_c(params);
    std::optional<CombineInside> inside;
    HipBackend* be = nullptr;
    engine::AlignResult r;
    try {
        if (!trace && !self_check && a_len > 0 && b_len > 0 && p.domain == engine::DomainKind::Full && p.doubling == engine::DoublingKind::None) {
            if (const int rc = align_full_matrix_cost(a, a_len, b, b_len, p, stats_out != nullptr, r)) return rc;
        } else {
            // Several callers inside at once, a parameter set the batch kernels take: one batch for all of them (combine_unit.hip)
            // (only callers that COULD be combined count as the crowd: a lone short-pair caller among many cost-only / long-pair /
            //  unsupported callers keeps the 2 ms single-pair path instead of a 300 us window plus a 6-8 ms batch)
            if (trace && !self_check && combine_eligible(a_len, b_len, params)) {
                inside.emplace();
                if (combine_align(a, a_len, b, b_len, params, cost_out, cigar_out, stats_out) == 0) return 0;
            }
            be = &pooled_backend();
            be->bind(a, a_len, b, b_len);
            if (!be->ok) return be->err ? be->err : PA_E_HIP;
            // pa_set_reference_cost_only(1) / PA_COST_ONLY_MODE=reference: trace == 0 runs the REFERENCE's cost-only arm (blocks.rs:252-277:
            // one block updated in place) through the host-driven engine over the HIP kernels -- the value the reference's
            // make_aligner(false) returns, upper bounds included (include/pa_astarpa2.h, DEVIATIONS.md)
            const bool ref_cost_only = !trace && reference_cost_only_requested();
            const bool no_sweep = ref_cost_only || std::getenv("PA_ENGINE_NO_SWEEP") != nullptr;  // (PA_ENGINE_NO_SWEEP: diagnostics / tests, the host-driven engine)
            const bool sweepable = !no_sweep && !self_check && sweep::sweep_supported(p, a_len, b_len);
            if (!sweepable || !align_sweep(p, *be, trace, r)) {
                if (sweepable) {
                    be->bind(a, a_len, b, b_len);  // fresh backend state for the host-driven engine
                    if (!be->ok) return be->err ? be->err : PA_E_HIP;
                }
                align_host_engine(p, *be, trace, /*traced_for_cost=*/!trace && sweepable, self_check, r);
            }
        }
    } catch (const engine::EnginePanic& e) {
        if (be && be->err) return be->err;
        set_error("astarpa2 engine panic: %s", e.what());
        return PA_E_INTERNAL;
    }
    if (cost_out) *cost_out = r.cost;
    if (cigar_out) *cigar_out = r.has_cigar ? r.cigar.to_string() : std::string();
    if (stats_out) engine::stats_to_c(r.stats, stats_out);
    return 0;
}

}  // namespace pa

using namespace pa;

// ---- device-resident operator handles (route 2 of INTEGRATION.md: the reference's engine over HIP operators) ------------------
// The sequences, the profile and the persistent h row of one pair stay on the GPU between calls; a call moves only the v
// words of its rectangle.  This is HipBackend behind a C handle.
struct pa_bp_ctx {
    HipBackend be;
    engine::BlockParams bp;
    int device = -1;  // the device its buffers and its stream live on
};
// A handle launches on the device it was created on: a call from a thread whose current device is another one is refused instead of
// launching there with pointers of this one.
static bool ctx_device_ok(const pa_bp_ctx* c, const char* what) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != c->device) {
        set_error("%s: the handle belongs to device %d, this thread's current device is %d (pa_set_device first)", what, c->device, cur);
        return false;
    }
    return true;
}

extern "C" pa_bp_ctx* pa_bp_ctx_create(const uint8_t* a, size_t n, const uint8_t* b, size_t m) {
    if (n > (size_t)(1u << 30) || m > (size_t)(1u << 30)) {
        set_error("sequence too long for i32 coordinates");
        return nullptr;
    }
    std::unique_ptr<pa_bp_ctx> c(new (std::nothrow) pa_bp_ctx());
    if (!c) {
        set_error("out of memory");
        return nullptr;
    }
    c->be.bind(a, n, b, m);
    if (!c->be.ok) return nullptr;
    (void)hipGetDevice(&c->device);
    try {
        c->be.enable_h_row();
    } catch (const engine::EnginePanic&) {
        return nullptr;
    }
    return c.release();
}

extern "C" int pa_bp_ctx_compute(pa_bp_ctx* c, int32_t i0, int32_t i1, size_t w0, size_t w1, uint64_t* v, int h_mode, int32_t* sum_out) {
    if (!c || i0 < 0 || i1 < i0 || i1 > c->be.n() || w1 < w0 || w1 > (size_t)((c->be.m() + 63) / 64) || (!v && w1 > w0) || h_mode < 0 || h_mode > 3) {
        set_error("pa_bp_ctx_compute: bad arguments");
        return PA_E_ARG;
    }
    if (!ctx_device_ok(c, "pa_bp_ctx_compute")) return PA_E_ARG;
    static_assert(sizeof(engine::V) == 16, "V is (p: u64, m: u64)");
    try {
        const engine::Cost s = c->be.compute(i0, i1, w0, w1, reinterpret_cast<engine::V*>(v), (engine::HMode)h_mode, c->bp);
        if (sum_out) *sum_out = s;
    } catch (const engine::EnginePanic&) {
        return c->be.err ? c->be.err : PA_E_INTERNAL;
    }
    return 0;
}

extern "C" int pa_bp_ctx_fill(pa_bp_ctx* c, int32_t i0, int32_t i1, size_t w0, size_t w1, uint64_t* v, uint64_t* values, int8_t* h_bottom) {
    if (!c || i0 < 0 || i1 < i0 || i1 > c->be.n() || w1 < w0 || w1 > (size_t)((c->be.m() + 63) / 64) || !v || !values) {
        set_error("pa_bp_ctx_fill: bad arguments");
        return PA_E_ARG;
    }
    if (!ctx_device_ok(c, "pa_bp_ctx_fill")) return PA_E_ARG;
    try {
        std::vector<int8_t> hb((size_t)(i1 - i0) + 1, 0);
        c->be.fill(i0, i1, w0, w1, reinterpret_cast<engine::V*>(v), reinterpret_cast<engine::V*>(values), hb.data(), c->bp);
        if (h_bottom) std::memcpy(h_bottom, hb.data(), (size_t)(i1 - i0));
    } catch (const engine::EnginePanic&) {
        return c->be.err ? c->be.err : PA_E_INTERNAL;
    }
    return 0;
}

extern "C" void pa_bp_ctx_destroy(pa_bp_ctx* c) { delete c; }

extern "C" void pa_params_nw(pa_astarpa2_params* p) { engine::params_to_c(engine::AstarPa2Params::nw(), p); }
extern "C" void pa_params_simple(pa_astarpa2_params* p) { engine::params_to_c(engine::AstarPa2Params::simple(), p); }
extern "C" void pa_params_full(pa_astarpa2_params* p) { engine::params_to_c(engine::AstarPa2Params::full(), p); }

extern "C" int pa_align(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, const pa_astarpa2_params* params,
                        int trace, int32_t* cost_out, char** cigar_out, pa_astarpa2_stats* stats_out) {
    if (!params) return PA_E_ARG;
    std::string cigar;
    const bool self_check = std::getenv("PA_ENGINE_SELF_CHECK") != nullptr;
    const int rc = align_hip(a, a_len, b, b_len, *params, trace != 0, self_check, cost_out, &cigar, stats_out);
    if (cigar_out) {
        *cigar_out = nullptr;
        if (rc == 0 && trace) {
            *cigar_out = (char*)std::malloc(cigar.size() + 1);
            if (!*cigar_out) {
                set_error("out of memory");
                return PA_E_NOMEM;
            }
            std::memcpy(*cigar_out, cigar.c_str(), cigar.size() + 1);
        }
    }
    return rc;
}
