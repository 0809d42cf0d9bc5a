// pa_batch.hpp -- the batched plan behind the C API's opaque `pa_batch` and the PA_ALIGN_PROFILE clock of its phases, for the host units
// that plan it: pa_hip.hip (creation, launch, report; it keeps the destructor's body) and apa2_jobs_unit.hip (the per-pair jobs of the
// batched A*PA2 modes).  No kernels.
#pragma once
#include "pa_hip_internal.hpp"
#include "slice_plan.hpp"
#include "apa2_units.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pa;  // pa_batch is the C API's type at global scope; what it is made of is pa's

// PA_ALIGN_PROFILE (diagnostics: where the time of a creation, an alignment call and a destruction goes), read once per process.
static bool align_profile() {
    static const bool on = getenv("PA_ALIGN_PROFILE") != nullptr;
    return on;
}

// The marks of PA_ALIGN_PROFILE on stderr: "[tag] what  ms since the mark before".  lap() is the figure alone.
struct PhaseClock {
    const char* tag;
    double t_mark = now();
    explicit PhaseClock(const char* tag_) : tag(tag_) {}
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    double lap() {
        const double t = now(), ms = t - t_mark;
        t_mark = t;
        return ms;
    }
    void mark(const char* what) {
        if (align_profile()) std::fprintf(stderr, "[%s] %-28s %8.3f ms\n", tag, what, lap());
    }
};

// ---- batched full DP ----------------------------------------------------------------------------

struct pa_batch {
    struct ReleaseScope {  // FIRST member = destroyed last: ends the scope the destructor's body opens (one device wait for all the buffers)
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~ReleaseScope() {
            release_scope_end();
            if (align_profile())
                std::fprintf(stderr, "[pa_batch_destroy] buffers released %.3f ms after the batch was created\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
    } release_scope_;
    size_t pairs = 0;
    std::vector<size_t> n, m, a_off, b_off, code_off, prof_off, gran_off;
    DeviceBuf d_a, d_b, d_codes, d_prof, d_v, d_gran, d_jobs, d_sums, d_misc, d_desc, d_wavelog;
    size_t max_n = 0, max_m = 0;
    std::vector<StripJob> jobs;
    std::vector<int> last_job;  // per pair (or -1 when w == 0)
    size_t total_gran = 0;
    bool gran_dirty = true;  // the hand-off granules must be cleared before the next pass
    int k = 1;  // 32-row subwords per lane of this batch's strips
    bool sequential = false;  // one wavefront per pair (pair_kernel) instead of chained strips
    int block_waves = 1;
    DeviceBuf d_first;  // sequential: first job of every pair (+ end)
    // big cost-only batches: groups of 32 pairs, bit-sliced (slice_kernel.hpp); the strips of `jobs` are not planned then
    slice::Plan* sliced = nullptr;
    // banded mode (pa_batch_create_banded): per-pair cost threshold of the diagonal band that was planned
    bool banded = false;
    std::vector<int32_t> band_t;
    size_t band_retries = 0;  // pairs re-run with a wider band (summed over passes)
    DeviceBuf d_rjobs, d_rfirst;  // retry sub-batches
    // traceback mode (pa_batch_create_trace / pa_batch_align)
    bool trace = false;
    int dt_max_g = 0, dt_fr_drop = 0;  // DT-trace options of the batched traceback (0: re-fill only)
    size_t trace_fallbacks = 0;  // pairs whose traceback was redone by the host engine
    std::vector<size_t> ckpt_off, cigar_off, word_off;  // per pair, in u32 (ckpt) / elements (cigar) / words of b before this pair
    DeviceBuf d_scratch_gran;
    DeviceBuf d_ckpt, d_cigar, d_cigar_len, d_costs, d_scratch_v, d_scratch_vals, d_tjobs, d_cig_src_off, d_packed;
    hipEvent_t ev2 = nullptr;
    uint8_t* h_text = nullptr;  // pinned host buffer for the packed CIGAR text of one chunk
    size_t h_text_size = 0;
    // pa_batch_align_view: the texts stay in h_text (one chunk) and the caller gets pointers + lengths; strings that come from elsewhere
    // (the host engine, the second round, the small-batch route, several chunks) are malloc'ed as usual and owned by the plan
    bool view_mode = false;
    std::vector<uint32_t> view_len;
    std::vector<char*> view_owned;
    bool in_text(const char* q) const { return h_text && (const uint8_t*)q >= h_text && (const uint8_t*)q < h_text + h_text_size; }
    void free_view_owned() {
        for (char* q : view_owned) std::free(q);
        view_owned.clear();
    }
    // pa_batch_align can work in CHUNKS of the (heaviest-first) order, each on a stream of its own: forward pass (batched A*PA2),
    // traceback, CIGAR text and its copy-out of different chunks overlap (one chunk by default: see the chunk plan in batch_create)
    static constexpr int kMaxChunks = 8;
    std::vector<int32_t> order_host;   // position -> pair (A*PA2: heaviest first; else the identity)
    std::vector<int32_t> torder_host;  // the same chunks with the pairs of a chunk in index order: what the traceback and the text kernels walk
                                       // (neighbouring pairs of the input in one workgroup: C4 traceback 10.0 against 10.9 ms in the forward order)
    DeviceBuf d_torder;
    DeviceBuf d_tlist;     // the traceback's own order: each chunk's pairs by descending cost (trace_order_kernel)
    uint32_t max_nm = 1;   // the longest |a| + |b| of the batch: no cost is larger
    std::vector<size_t> chunk_lo;      // chunk c = positions [chunk_lo[c], chunk_lo[c + 1])
    std::vector<uint64_t> chunk_base;  // byte offset of chunk c's region of d_packed
    hipStream_t cstream[kMaxChunks] = {};
    hipEvent_t ev_pre = nullptr, evF0[kMaxChunks] = {}, evF1[kMaxChunks] = {}, evT1[kMaxChunks] = {};
    DeviceBuf d_cmeta, d_tlen_pos, d_dst_pos;  // d_cmeta: u64 text totals [kMaxChunks], then u32 tickets [kMaxChunks]
    uint8_t* h_meta = nullptr;                  // pinned: u64 totals [kMaxChunks], u32 tlen [pairs], u64 dst [pairs]
    size_t h_meta_size = 0;
    // A*PA2 mode (pa_batch_create_params): one wavefront runs the whole band search of a pair (apa2_kernel.hpp); d_ckpt is the
    // pairs' column store, the traceback reads the blocks of the successful pass from it
    bool astar = false;
    // the block-column store is band-proportional: slot width per pair in words (sweep_logic.hpp SlotGeom); a pair whose band leaves its
    // window is aligned again with full-height slots (second round of pa_batch_align)
    std::vector<uint32_t> win_words, slot_ratio;
    int window_override = -1;  // -1: the policy below; 0: full columns; > 0: that many words
    size_t window_retries = 0;
    double window_retry_peak_bytes = 0;  // the largest full-height block-column store a second round of this plan held at a time
    pa_astarpa2_params aparams_c{};
    apa2::SearchParams sp{};
    DeviceBuf d_rec, d_results, d_pjobs, d_order, d_tstats, d_sh;
    DeviceBuf d_sketch;  // [pairs] the divergence sketch (sketch_unit.hip), kept so that it is released with the batch's other buffers
    DeviceBuf d_rdv;  // 8 x u64: the rendezvous of half-wave blocks in the last forward pass (strips run fused, served by a partner, alone, withdrawn)
    // ... the whole family (pa_batch_create_params with GCSH / pruning / incremental doubling: apa2_full_kernel.hpp)
    bool astar_full = false;
    apa2::FullParams fsp{};
    DeviceBuf d_fjobs, d_jh, d_hrow, d_mi, d_mj, d_active, d_win, d_win0, d_lrec, d_cell, d_probe;
    size_t full_matches = 0, full_seeds = 0;
    double full_build_ms = 0;  // host time spent on the matches of the heuristic (reporting; 0 when the GPU finds them)
    // the matches found on the GPU (gcsh_build_kernel.hpp), inside every pa_batch_align / pa_batch_run
    bool device_build = false;
    DeviceBuf d_bjobs, d_bscratch, d_bstatus, d_bticket;
    hipEvent_t evB0 = nullptr, evB1 = nullptr;
    std::vector<pa_astarpa2_stats> pair_stats;  // of the last pa_batch_align
    double apa2_strip_instr = 0;  // modelled VALU instructions of the DP strips of the last pa_batch_align (reporting)
    double cells = 0, word_updates = 0, algo_bytes = 0;
    hipStream_t stream = nullptr;
    // INVARIANT (round 6, replaces a flag nothing ever set): everything that reads or writes this batch's buffers is queued on `stream` or on
    // one of cstream[] -- never on the null stream or a stream of another object.  The destructor relies on it: it waits for these streams
    // only and hands the buffers to the cache, where another thread may take them at once.  PA_POISON_ALLOC runs keep it honest.
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~pa_batch();  // pa_hip.hip
};

// Pair i's two sequences, back from the device (an empty one is not copied).
bool fetch_pair(const pa_batch* p, size_t i, std::vector<uint8_t>& a, std::vector<uint8_t>& b);

// pa_hip.hip, for apa2_jobs_unit.hip (TraceJob is trace_kernel.hpp's, which a unit without kernels cannot include): what the batched
// A*PA2 modes add to pair i's trace job -- its banded blocks, its result, its statistics and the geometry of its column store.
namespace pa {
struct TraceJob;
}
void fill_trace_job(std::vector<TraceJob>& tjobs, const pa_batch* p, size_t i, const sweep::BlockRec* rec, const apa2::PairResult* result);
// apa2_jobs_unit.hip: the per-pair jobs of a batched A*PA2 plan (apa2_kernel.hpp's PairJob or apa2_full_kernel.hpp's FullJob by
// p->astar_full), their buffers, the start order; completes the trace jobs.
bool apa2_make_jobs(pa_batch* p, const uint8_t* const* a, const uint8_t* const* b, std::vector<TraceJob>& tjobs);
