// sweep_hip.hpp -- the HIP launcher of the device-side sweep: one launch per align_for_bounded_dist pass (sweep_wave.hpp).
//
// Included by engine_hip.hip only: the sweep kernels (sweep_kernel.hpp) are instantiated in that translation unit.
#pragma once
#include <atomic>
#include <memory>
#include <vector>

#include "hip_backend.hpp"
#include "sweep_host.hpp"
#include "sweep_kernel.hpp"

namespace pa {

// Launcher of sweep::SweepAligner over HIP.  Its buffers are pooled per host thread like the backend's.
// Passes of one band search run pipelined (sweep_host.hpp search()): every pass in flight has a SLOT with its own records,
// buffers and stream; the merged block records of the completed passes alternate between two arrays.
struct SweepSlot {
    DeviceBuf d_brec, d_trec, d_misc, d_start, d_pring, d_gran, d_col;
    DeviceBuf d_merged;  // the block records of every earlier pass with this pass's on top (what the next pass reads once this one is over)
    hipStream_t s = nullptr;
    hipEvent_t merged_ev = nullptr;  // recorded behind the merge of the pass that ran here
    sweep::Status* h_status = nullptr;  // pinned
    // the pass that runs (or ran last) here
    int seq = 0;
    uint32_t pass = 0;
    bool live = false;
    int32_t f_max = 0, waves = 0;
    sweep::PassGeometry geo{};
    double t_launch = 0;
    // bprog @0, ticket @16, done @24, merge counter @32, cancel @56 (directly before the status block), status @64, phase clocks @512
    uint64_t* bprog() { return d_misc.as<uint64_t>(); }
    uint32_t* ticket() { return d_misc.as<uint32_t>() + 4; }
    uint64_t* done() { return d_misc.as<uint64_t>() + 3; }
    uint32_t* merge_count() { return d_misc.as<uint32_t>() + 8; }
    uint64_t* cancel() { return d_misc.as<uint64_t>() + 7; }
    sweep::Status* status() { return reinterpret_cast<sweep::Status*>(d_misc.as<uint8_t>() + 64); }
};
struct SweepPool {
    // a pass's records must outlive its successor, and a pass that is taken again (see sweep_host.hpp) follows a pass that was
    // completed five launches earlier: two slots more than passes in flight
    static constexpr int kSlots = 7;
    static constexpr int kMaxInFlight = 5;
    SweepSlot slots[kSlots];
    DeviceBuf d_merged0, d_sh, d_recs, d_offs, d_pack;  // d_merged0: "no block exists yet" (what the first pass of a pair reads)
    // hipFree waits for the whole device -- with passes in flight that serialises them (C5 cold: 2.7 s instead of 1.x).  A slot
    // buffer that has to grow while other passes run is therefore replaced, and the old allocation freed when nothing is in flight.
    std::vector<void*> graveyard;
    void bury(DeviceBuf& b) {
        if (b.ptr) graveyard.push_back(b.ptr);
        b.ptr = nullptr;
        b.size = 0;
    }
    void free_graveyard() {
        for (void* q : graveyard) (void)hipFree(q);
        graveyard.clear();
    }
    hipStream_t ctl = nullptr;  // cancel words go out here, past the running passes
    PinnedBuf pinned;  // read_blocks' records and packed columns
    uint32_t pass_id = 0;
    int device = -1;
    bool ok = false;
    SweepPool() {
        ok = hip_ok(hipStreamCreateWithFlags(&ctl, hipStreamNonBlocking), "hipStreamCreate");
        for (SweepSlot& sl : slots)
            ok = ok && hip_ok(hipStreamCreateWithFlags(&sl.s, hipStreamNonBlocking), "hipStreamCreate") &&
                 hip_ok(hipEventCreateWithFlags(&sl.merged_ev, hipEventDisableTiming), "hipEventCreate") &&
                 hip_ok(hipHostMalloc((void**)&sl.h_status, sizeof(sweep::Status), hipHostMallocDefault), "hipHostMalloc");
    }
    ~SweepPool() {
        free_graveyard();
        pinned.release();
        for (SweepSlot& sl : slots) {
            if (sl.h_status) (void)hipHostFree(sl.h_status);
            if (sl.merged_ev) (void)hipEventDestroy(sl.merged_ev);
            if (sl.s) (void)hipStreamDestroy(sl.s);
        }
        if (ctl) (void)hipStreamDestroy(ctl);
    }
};
static std::unique_ptr<SweepPool>& sweep_pool_slot() {
    static thread_local std::unique_ptr<SweepPool> tl;
    return tl;
}
static SweepPool& sweep_pool() {
    std::unique_ptr<SweepPool>& tl = sweep_pool_slot();
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!tl || tl->device != dev) {
        tl = std::make_unique<SweepPool>();
        tl->device = dev;
    }
    return *tl;
}

struct HipSweepLauncher {
    HipBackend& be;
    SweepPool& pool;
    int32_t n = 0, m = 0, nblk = 0;
    bool trace = false;
    bool has_sh = false;
    int32_t heur_kind = sweep::kHeurGap;

    HipSweepLauncher(HipBackend& backend, SweepPool& p) : be(backend), pool(p) { active_callers().fetch_add(1, std::memory_order_relaxed); }
    ~HipSweepLauncher() {
        cancel_after(0);
        active_callers().fetch_sub(1, std::memory_order_relaxed);
    }
    HipSweepLauncher(const HipSweepLauncher&) = delete;
    HipSweepLauncher& operator=(const HipSweepLauncher&) = delete;

    void hip_fail(const char* what) { throw sweep::SweepFallback(what, -2); }
    static bool timing_on() {
        static const bool on = std::getenv("PA_SWEEP_TIMING") != nullptr;
        return on;
    }
    SweepSlot& slot_of(int seq) { return pool.slots[seq % SweepPool::kSlots]; }
    // (a pass's records must outlive its successor, which reads them: one slot more than passes in flight)
    // Passes in flight run on separate streams, and streams only run side by side on separate hardware queues: the ROCm runtime
    // multiplexes all streams of a process over GPU_MAX_HW_QUEUES of them (default 4; pa_runtime_hints() below asks for 16
    // when the library is loaded before the runtime starts).  A pass queued BEHIND a later one would only cost time, never
    // correctness: passes are submitted in order and wait for their predecessors only.
    // Every pass in flight is a RUNNING kernel (it polls its predecessor) on a stream of its own, and the GPU serves only so many
    // queues side by side: with five passes each, four host threads got 716 pairs/s out of the drop-in loop (10 kbp pairs), with
    // two each 1042; eight threads 698 -> 1489 (profiles/r02_runs/dropin_threads.log).  Short pairs rarely need more than three
    // tries, passes beyond that are launches and cancellations for nothing.
    int max_in_flight() const {
        static const int forced = [] {
            const char* e = std::getenv("PA_SWEEP_DEPTH");
            return e ? std::min(std::max(std::atoi(e), 1), SweepPool::kMaxInFlight) : 0;
        }();
        if (forced) return forced;
        static const int queues = [] {
            const char* q = std::getenv("GPU_MAX_HW_QUEUES");
            return q ? std::max(std::atoi(q), 1) : 4;
        }();
        const int base = queues >= 8 ? (nblk > kShortPairBlocks ? SweepPool::kMaxInFlight : 3) : 3;
        const int callers = recent_callers();
        return callers == 1 ? base : (callers == 2 ? std::min(base, 3) : 2);
    }
    // The callers inside an alignment now, or the most seen during the last 20 ms: a thread between two calls of a loop still counts.
    static int recent_callers() {
        static std::atomic<int> peak{0};
        static std::atomic<int64_t> peak_ns{0};
        const int now_callers = std::max(active_callers().load(std::memory_order_relaxed), 1);
        const int64_t now = (int64_t)(engine::now_s() * 1e9);
        if (now_callers >= peak.load(std::memory_order_relaxed) || now - peak_ns.load(std::memory_order_relaxed) > 20'000'000) {
            peak.store(now_callers, std::memory_order_relaxed);  // (racing updates can only misjudge the depth for a moment)
            peak_ns.store(now, std::memory_order_relaxed);
        }
        return std::max(now_callers, peak.load(std::memory_order_relaxed));
    }
    static constexpr int32_t kShortPairBlocks = 128;  // 32 kbp
    static std::atomic<int>& active_callers() {  // host threads inside a sweep alignment right now
        static std::atomic<int> n{0};
        return n;
    }
    // wavefronts: one per strip the band can cover at a time (+ slack), one workgroup each
    int pass_waves(int32_t f_max) const {
        const sweep::PassGeometry g = sweep::pass_geometry(n, m, f_max);
        int64_t waves = (2ll * g.win) / sweep::kStripRows + 6;
        if (waves > g.nstrips) waves = g.nstrips;
        if (waves > 1024) waves = 1024;
        return (int)waves;
    }
    // Wavefronts of all passes in flight.  Most of a pass's wavefronts idle (a pass reserves one per strip its window can hold,
    // the band covers a fraction of them at a time), so somewhat more than one per SIMD is fine; far more would only slow
    // the passes that matter.
    int wave_budget() const {
        static const int budget = std::getenv("PA_SWEEP_WAVE_BUDGET") ? std::atoi(std::getenv("PA_SWEEP_WAVE_BUDGET")) : 1600;  // (C5: 1024 -> 1.9 s, 1600 -> 1.5 s, 4096 -> 4.9 s)
        return budget;
    }

    // bytes of a zero-initialised tagged buffer: cleared only when it is new (tags of older passes never match)
    void reserve_tagged(DeviceBuf& b, size_t bytes, hipStream_t st) {
        if (reserve_no_sync(b, bytes) && !hip_ok(hipMemsetAsync(b.ptr, 0, b.size, st), "memset")) hip_fail("memset");
    }
    // grow-only, never a hipFree (see SweepPool::graveyard); true when a new, uninitialised buffer was allocated
    bool reserve_no_sync(DeviceBuf& b, size_t bytes) {
        if (b.ptr && b.size >= bytes) return false;
        pool.bury(b);
        if (!b.alloc(bytes + bytes / 4 + 256)) hip_fail("hipMalloc");
        return true;
    }

    void begin_pair(int32_t n_, int32_t m_, int32_t nblk_, const int32_t* sh, bool tr) {
        using namespace sweep;
        if (!pool.ok) hip_fail("sweep pool");
        pool.free_graveyard();  // (nothing is in flight between pairs)
        n = n_;
        m = m_;
        nblk = nblk_;
        trace = tr;
        has_sh = sh != nullptr;
        const size_t recs = (size_t)nblk + 2;
        if (pool.pass_id >= 3000) {  // tags wrap at 4095: start over with clean tagged buffers (nothing is in flight between pairs)
            for (SweepSlot& sl : pool.slots)
                for (DeviceBuf* b : {&sl.d_brec, &sl.d_trec, &sl.d_start, &sl.d_pring, &sl.d_misc})
                    if (b->ptr && !hip_ok(hipMemsetAsync(b->ptr, 0, b->size, be.s), "memset")) hip_fail("memset");
            pool.pass_id = 0;
        }
        if (!pool.d_merged0.reserve(recs * sizeof(BlockRec)) ||
            !hip_ok(hipMemsetD32Async((hipDeviceptr_t)pool.d_merged0.ptr, (int)kNone, recs * sizeof(BlockRec) / 4, be.s), "memset merged"))
            hip_fail("merged records");
        for (SweepSlot& sl : pool.slots) {
            if (!sl.d_merged.reserve(recs * sizeof(BlockRec))) hip_fail("merged records");
            reserve_tagged(sl.d_brec, recs * sizeof(BRec), be.s);
            reserve_tagged(sl.d_trec, recs * sizeof(TRec), be.s);
            reserve_tagged(sl.d_misc, 1024, be.s);
            sl.live = false;
            sl.seq = 0;
        }
        if (has_sh) {
            if (!pool.d_sh.reserve(((size_t)n + 1) * 4) ||
                !hip_ok(hipMemcpyAsync(pool.d_sh.ptr, sh, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, be.s), "H2D sh"))
                hip_fail("sh table");
        }
        // the passes run on the slots' streams: everything set up on the pair's stream (profiles, codes, the above) is done first
        if (!hip_ok(hipStreamSynchronize(be.s), "sync")) hip_fail("begin_pair");
    }

    sweep::BlockRec read_merged(int seq, int32_t k) {  // after wait_pass(seq)
        sweep::BlockRec r;
        const DeviceBuf& mb = seq == 0 ? pool.d_merged0 : slot_of(seq).d_merged;
        if (seq != 0 && slot_of(seq).seq != seq) hip_fail("merged records of a pass whose slot was reused");
        if (!hip_ok(hipMemcpyAsync(&r, mb.as<sweep::BlockRec>() + k, sizeof(r), hipMemcpyDeviceToHost, be.s), "D2H rec") ||
            !hip_ok(hipStreamSynchronize(be.s), "sync"))
            hip_fail("read_merged");
        return r;
    }

    // A pass in three pieces, all on the slot's stream: its buffers, the init kernel, then sweep + merge + event.
    void launch_pass(int seq, int prev_seq, int32_t f_max, int32_t sparse_h, const sweep::PassInit& init) {
        using namespace sweep;
        SweepSlot& sl = slot_of(seq);
        if (sl.live) hip_fail("sweep slot busy");
        SweepSlot* pv = prev_seq ? &slot_of(prev_seq) : nullptr;
        if (pv && (pv == &sl || pv->seq != prev_seq)) hip_fail("sweep slot of the previous pass was reused");
        // tags carry 12 bits of pass id (sweep_logic.hpp blk_tag) and the tagged buffers are cleared between pairs only: a pair that
        // needs more passes than that (LinearSearch with a small delta) goes to the host-driven engine instead of aliasing tags
        if (pool.pass_id >= 4000) throw SweepFallback("pass ids exhausted within one pair", -4);
        pool.pass_id += 1;
        sl.seq = seq;
        sl.pass = pool.pass_id;
        sl.f_max = f_max;
        sl.geo = pass_geometry(n, m, f_max);
        const size_t gran_bytes = size_slot_buffers(sl);
        launch_init(sl, init, gran_bytes);
        launch_sweep_and_merge(sl, pv, sparse_h);
        sl.live = true;
    }

    // The slot's buffers for the geometry of its pass; returns the bytes of its hand-off granules.
    size_t size_slot_buffers(SweepSlot& sl) {
        const sweep::PassGeometry& geo = sl.geo;
        const size_t nslots = trace ? (size_t)nblk + 1 : (size_t)geo.col_ring;
        const size_t gran_bytes = (size_t)geo.nstrips * (size_t)geo.gran_stride * 8;
        const size_t col_bytes = nslots * (size_t)geo.col_stride * 16;
        const size_t pr_bytes = (size_t)geo.nstrips * (size_t)geo.pr_stride * 8;
        if (gran_bytes + col_bytes + pr_bytes > (size_t)40 << 30) throw sweep::SweepFallback("sweep buffers too large", -3);
        reserve_tagged(sl.d_start, (size_t)geo.nstrips * 8, sl.s);
        reserve_tagged(sl.d_pring, pr_bytes, sl.s);
        (void)reserve_no_sync(sl.d_gran, gran_bytes);
        (void)reserve_no_sync(sl.d_col, col_bytes);
        return gran_bytes;
    }

    void launch_init(SweepSlot& sl, const sweep::PassInit& init, size_t gran_bytes) {
        using namespace sweep;
        InitArgs ia;
        ia.brec = sl.d_brec.as<BRec>();
        ia.trec = sl.d_trec.as<TRec>();
        ia.bprog = sl.bprog();
        ia.strip_start = sl.d_start.as<uint64_t>();
        ia.status = sl.status();
        ia.ticket = sl.ticket();
        ia.pass = sl.pass;
        ia.js1 = init.js1;
        ia.je1 = init.je1;
        ia.ojs1 = init.ojs1;
        ia.oje1 = init.oje1;
        ia.flags1 = init.flags1;
        ia.top1 = init.top1;
        ia.fs0 = init.fs0;
        ia.last_strip = init.last_strip;
        ia.nstrips = sl.geo.nstrips;
        // workgroup 0 sets the pass up, all of them clear the hand-off granules (16 words per thread and round); a large granule
        // buffer (long pairs: a pass takes milliseconds, a launch more does not matter) is left to the runtime's fill kernel
        ia.gran = sl.d_gran.as<uint64_t>();
        ia.gran_words = gran_bytes / 8;
        if (gran_bytes > ((size_t)4 << 20)) {
            ia.gran_words = 0;
            if (!hip_ok(hipMemsetAsync(sl.d_gran.ptr, 0, gran_bytes, sl.s), "memset granules")) hip_fail("memset");
        }
        const uint64_t init_groups = std::min<uint64_t>(std::max<uint64_t>(ia.gran_words / ((uint64_t)kInitThreads * 16), 1), 2048);
        hipLaunchKernelGGL(sweep_init_kernel, dim3((unsigned)init_groups), dim3(kInitThreads), 0, sl.s, ia);
    }

    // `pv`: the slot of the previous pass (nullptr for the first pass of a pair).
    void launch_sweep_and_merge(SweepSlot& sl, SweepSlot* pv, int32_t sparse_h) {
        using namespace sweep;
        const PassGeometry& geo = sl.geo;
        const bool pv_running = pv && pv->live;  // still in flight: read its records as they appear; else only its merged array
        const BlockRec* merged_in = pv ? pv->d_merged.as<BlockRec>() : pool.d_merged0.as<BlockRec>();
        Ctx c;
        c.a_codes = be.d_codes.as<uint32_t>();
        c.b_prof = be.d_prof.as<uint32_t>();
        c.n = n;
        c.m = m;
        c.nblk = nblk;
        c.wtot = geo.wtot;
        c.f_max = sl.f_max;
        c.pass = sl.pass;
        c.heur = heur_kind;
        c.sparse_h = sparse_h;
        c.sh_h = has_sh ? pool.d_sh.as<int32_t>() : nullptr;
        c.store_cols = trace ? 1 : 0;
        c.d_old = merged_in;
        c.prev_brec = pv_running ? pv->d_brec.as<BRec>() : nullptr;
        c.prev_pass = pv_running ? pv->pass : 0;
        c.prev_done = pv_running ? pv->done() : sl.done();
        c.cancel = sl.cancel();
        c.brec = sl.d_brec.as<BRec>();
        c.trec = sl.d_trec.as<TRec>();
        c.bprog = sl.bprog();
        c.strip_start = sl.d_start.as<uint64_t>();
        c.pring = sl.d_pring.as<uint64_t>();
        c.pr_stride = geo.pr_stride;
        c.gran = sl.d_gran.as<uint64_t>();
        c.gran_stride = geo.gran_stride;
        c.win = geo.win;
        c.col = sl.d_col.as<uint64_t>();
        c.col_stride = geo.col_stride;
        c.col_ring = geo.col_ring;
        c.status = sl.status();
        c.ticket = sl.ticket();
        c.nstrips = geo.nstrips;
        c.nwaves = pass_waves(sl.f_max);
        sl.waves = c.nwaves;
        c.spin_limit = 1u << 19;  // ~2 s of backed-off polls
        c.timing = nullptr;
        if (timing_on()) {
            c.timing = sl.d_misc.as<uint64_t>() + 64;  // bytes 512..575 of d_misc
            (void)hipMemsetAsync(c.timing, 0, 64, sl.s);
            sl.t_launch = engine::now_s();
        }
        hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)c.nwaves), dim3(64), 0, sl.s, c);
        // behind the pass: merge its records into the older ones (after the previous pass's merge); the same launch then publishes
        // the done word and writes the status into the pinned copy that wait_pass reads
        if (pv_running && !hip_ok(hipStreamWaitEvent(sl.s, pv->merged_ev, 0), "hipStreamWaitEvent")) hip_fail("event");
        hipLaunchKernelGGL(sweep_merge_kernel, dim3((unsigned)((nblk + 2 + 255) / 256)), dim3(256), 0, sl.s, sl.d_brec.as<BRec>(), merged_in,
                           sl.d_merged.as<BlockRec>(), sl.status(), nblk, sl.merge_count(), sl.done(), sl.pass, sl.h_status);
        if (!hip_ok(hipEventRecord(sl.merged_ev, sl.s), "hipEventRecord") || !hip_ok(hipGetLastError(), "sweep launch")) hip_fail("sweep pass");
    }

    sweep::Status wait_pass(int seq) {
        SweepSlot& sl = slot_of(seq);
        if (sl.seq != seq) hip_fail("sweep slot lost");
        if (!hip_ok(hipStreamSynchronize(sl.s), "sync")) hip_fail("sweep pass");
        sl.live = false;
        const sweep::Status st = *sl.h_status;
        if (timing_on()) {
            uint64_t tm[8] = {0};
            (void)hipMemcpy(tm, sl.d_misc.as<uint64_t>() + 64, 64, hipMemcpyDeviceToHost);
            std::fprintf(stderr, "sweep pass %u (seq %d): f_max=%d waves=%d state=%u value=%d k_end=%d  %.3f ms after its launch | strip-us: begin %.0f slow %.0f cross %.0f (probes %.0f) end %.0f bottom %.0f plain %.0f gran %.0f flush %.0f\n",
                         sl.pass, seq, sl.f_max, sl.waves, st.state, st.value, st.k_end, (engine::now_s() - sl.t_launch) * 1e3, tm[0] * 0.01, tm[1] * 0.01,
                         tm[6] * 0.01, tm[7] * 0.01, tm[2] * 0.01, tm[3] * 0.01, tm[4] * 0.01, (double)(tm[5] & 0xFFFFFFFFull) * 0.01, (double)(tm[5] >> 32) * 0.01);
        }
        return st;
    }

    // (short pairs: the speculative passes' wavefronts are few and the traceback's kernels small; on C3 waiting first measured better)
    bool cancel_without_waiting() const {
        static const bool off = std::getenv("PA_SWEEP_CANCEL_WAIT") != nullptr;
        return !off && nblk <= kShortPairBlocks;
    }
    // Give up every launched pass behind `seq` and wait until they (and their merges) are gone.
    void cancel_after(int seq, bool wait = true) {
        bool any = false;
        for (SweepSlot& sl : pool.slots)
            if (sl.live && sl.seq > seq) {
                any = hip_ok(hipMemsetD32Async((hipDeviceptr_t)sl.cancel(), (int)sl.pass, 1, pool.ctl), "cancel") || any;
            }
        if (!any || !wait) return;
        (void)hipStreamSynchronize(pool.ctl);
        for (int q = seq + 1; q <= seq + SweepPool::kSlots; ++q) {  // in launch order
            SweepSlot& sl = slot_of(q);
            if (!sl.live || sl.seq <= seq) continue;
            (void)hipStreamSynchronize(sl.s);
            sl.live = false;
        }
    }

    // The blocks of the pass that just succeeded, for Blocks::trace.
    void read_blocks(int seq, std::vector<engine::Block>& blocks) {
        using namespace sweep;
        SweepSlot& sl = slot_of(seq);
        const size_t recs = (size_t)nblk + 1;
        if (!pool.d_recs.reserve(recs * sizeof(BlockOut)) || !pool.d_offs.reserve(recs * 8)) hip_fail("hipMalloc");
        // A block's column holds at most col_stride words, so the packed columns fit a pinned buffer of nblk * col_stride words: up to
        // 16 MB of them the one-synchronisation route, beyond (Mbp pairs) the two-step route, which sizes the buffer by what the records
        // say.  PA_SWEEP_READ_TWO_STEP (tests): the two-step route at every size.
        static const bool two_step = std::getenv("PA_SWEEP_READ_TWO_STEP") != nullptr;
        const size_t bound_words = (size_t)nblk * (size_t)sl.geo.col_stride;
        if (!two_step && bound_words * 16 <= (size_t(16) << 20)) read_blocks_pinned(sl, bound_words, blocks);
        else read_blocks_two_step(sl, blocks);
    }

    static size_t block_words(const sweep::BlockOut& o) { return (size_t)(o.je - o.js) / 64; }
    // Block k as the engine keeps it, from its record and its packed column.
    void set_block(engine::Block& bl, int32_t k, const sweep::BlockOut& o, const uint64_t* words) {
        bl.i_range = engine::IRange{(k - 1) * sweep::kBlockW, k * sweep::kBlockW < n ? k * sweep::kBlockW : n};
        bl.original_j_range = engine::JRange{o.ojs, o.oje};
        bl.j_range = engine::JRange{o.js, o.je};
        bl.fixed_j_range = engine::JRange{o.fs, o.fe};
        bl.offset = o.js;
        bl.top_val = o.top_val;
        bl.bot_val = o.bot_val;
        bl.j_h.reset();
        bl.v.resize(block_words(o));
        std::memcpy(bl.v.data(), words, block_words(o) * 16);
    }

    // One synchronisation: the gather kernel writes records and packed columns directly into a pinned buffer sized by the bound.
    void read_blocks_pinned(SweepSlot& sl, size_t bound_words, std::vector<engine::Block>& blocks) {
        using namespace sweep;
        const size_t recs = (size_t)nblk + 1;
        const size_t off_cols = (recs * sizeof(BlockOut) + 63) & ~size_t(63);
        uint8_t* hb = static_cast<uint8_t*>(pool.pinned.reserve(off_cols + bound_words * 16 + 64));
        if (!hb) hip_fail("pinned");
        BlockOut* hrp = reinterpret_cast<BlockOut*>(hb);
        uint64_t* hp = reinterpret_cast<uint64_t*>(hb + off_cols);
        hipLaunchKernelGGL(sweep_records_offsets_kernel, dim3(1), dim3(1024), 0, be.s, sl.d_brec.as<BRec>(), pool.d_recs.as<BlockOut>(), hrp,
                           pool.d_offs.as<int64_t>(), nblk);
        hipLaunchKernelGGL(sweep_gather_kernel, dim3((unsigned)nblk), dim3(256), 0, be.s, sl.d_col.as<uint64_t>(), sl.geo.col_stride, sl.geo.win,
                           pool.d_recs.as<BlockOut>(), pool.d_offs.as<int64_t>(), hp, nblk);
        if (!hip_ok(hipGetLastError(), "sweep gather launch") || !hip_ok(hipStreamSynchronize(be.s), "sync")) hip_fail("columns");
        size_t at = 0;
        for (int32_t k = 1; k <= nblk; ++k) {
            const BlockOut o = hrp[(size_t)k];
            if (at + block_words(o) > bound_words) hip_fail("sweep columns beyond their bound");
            set_block(blocks[(size_t)k], k, o, hp + at * 2);
            at += block_words(o);
        }
    }

    // Records first, then a buffer of exactly the words they announce: two synchronisations.
    void read_blocks_two_step(SweepSlot& sl, std::vector<engine::Block>& blocks) {
        using namespace sweep;
        const size_t recs = (size_t)nblk + 1;
        hipLaunchKernelGGL(sweep_records_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, be.s, sl.d_brec.as<BRec>(),
                           pool.d_recs.as<BlockOut>(), nblk);
        std::vector<BlockOut> hr(recs);
        if (!hip_ok(hipMemcpyAsync(hr.data(), pool.d_recs.ptr, recs * sizeof(BlockOut), hipMemcpyDeviceToHost, be.s), "D2H records") ||
            !hip_ok(hipStreamSynchronize(be.s), "sync"))
            hip_fail("records");
        std::vector<int64_t> offs(recs, 0);
        int64_t total = 0;
        for (int32_t k = 1; k <= nblk; ++k) {
            offs[(size_t)k] = total;
            total += (int64_t)block_words(hr[(size_t)k]);
        }
        if (!pool.d_pack.reserve((size_t)total * 16 + 16)) hip_fail("hipMalloc");
        uint64_t* hp = static_cast<uint64_t*>(pool.pinned.reserve((size_t)total * 16 + 16));
        if (!hp) hip_fail("pinned");
        if (!hip_ok(hipMemcpyAsync(pool.d_offs.ptr, offs.data(), recs * 8, hipMemcpyHostToDevice, be.s), "H2D offsets")) hip_fail("offsets");
        hipLaunchKernelGGL(sweep_gather_kernel, dim3((unsigned)nblk), dim3(256), 0, be.s, sl.d_col.as<uint64_t>(), sl.geo.col_stride, sl.geo.win,
                           pool.d_recs.as<BlockOut>(), pool.d_offs.as<int64_t>(), pool.d_pack.as<uint64_t>(), nblk);
        if (!hip_ok(hipMemcpyAsync(hp, pool.d_pack.ptr, (size_t)total * 16, hipMemcpyDeviceToHost, be.s), "D2H columns") ||
            !hip_ok(hipStreamSynchronize(be.s), "sync"))
            hip_fail("columns");
        for (int32_t k = 1; k <= nblk; ++k) set_block(blocks[(size_t)k], k, hr[(size_t)k], hp + offs[(size_t)k] * 2);
    }
};

}  // namespace pa
