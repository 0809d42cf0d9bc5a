// hip_backend.hpp -- HipBackend: the engine's compute / fill operators (engine.hpp's Backend concept) over the HIP strip kernels.
//
// HipBackend keeps the pair's profile (packed codes of a, BitProfile words of b) and the persistent
// horizontal-delta row (one byte per column, blocks.rs:103-105) resident on the GPU; every
// compute / fill rectangle of the engine is one chained-strip launch of strip_kernel.  Block right-edge
// columns (`Block::v`) live in host memory because the band logic reads them (Block::index).
//
// Included by engine_hip.hip only: the rectangle kernels it launches are instantiated in that translation unit.
#pragma once
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine.hpp"
#include "pa_hip_internal.hpp"

namespace pa {

using engine::BlockParams;
using engine::Cost;
using engine::HMode;
using engine::I;
using engine::V;

constexpr size_t strips_of(size_t words) { return (words + kWordsPerStrip - 1) / kWordsPerStrip; }
// a byte of the h row (bit 0: +1, bit 1: -1) as the delta it stands for
inline int h_delta(uint8_t x) { return (x & 1) - ((x >> 1) & 1); }

struct HipBackend {
    std::vector<uint8_t> a_, b_;
    DeviceBuf d_a, d_b, d_codes, d_prof, d_h, d_htmp, d_gran, d_call, d_misc, d_values;
    size_t w_total = 0;
    hipStream_t s = nullptr;
    bool ok = false;
    int err = 0;
    bool has_h = false;
    PinnedBuf h_stage;  // pinned staging
    // host-mapped mailbox of the per-block fast path: [done, err, sum, pad.. | v words]
    uint8_t* mbox = nullptr;      // host address
    uint8_t* mbox_dev = nullptr;  // the same memory as the GPU sees it
    size_t mbox_size = 0;
    uint32_t seq = 0;
    DeviceBuf d_counter;
    size_t gran_zeroed = 0;  // granules of d_gran known to be zero (the strips hand every granule back zeroed)

    int device = -1;  // the device the pooled buffers live on

    HipBackend() = default;
    HipBackend(const uint8_t* a, size_t n, const uint8_t* b, size_t m) { bind(a, n, b, m); }

    // (Re)bind the backend to a pair.  Buffers, the stream and the mailbox are kept from call to call (a thread-local pool,
    // see pooled_backend()): a relinked astarpa-c user calls astarpa2_simple in a loop, and six hipMallocs + a stream per
    // call cost more than a short alignment.
    void bind(const uint8_t* a, size_t n, const uint8_t* b, size_t m) {
        ok = false;
        err = 0;
        has_h = false;
        a_.assign(a, a + n);
        b_.assign(b, b + m);
        if (!ensure_device()) { err = PA_E_HIP; return; }
        (void)hipGetDevice(&device);
        w_total = (m + 63) / 64;
        const size_t cw = (n + 15) / 16 + 16;  // the sweep kernel reads up to 8 words past the last column's
        if (!d_a.reserve(n) || !d_b.reserve(m) || !d_codes.reserve(cw * 4) || !d_prof.reserve(w_total * 16 + 16) ||
            !d_misc.reserve(16) || !d_htmp.reserve(n + 64)) { err = PA_E_HIP; return; }
        if (!s && !hip_ok(hipStreamCreate(&s), "hipStreamCreate")) { err = PA_E_HIP; return; }
        // The per-call set-up in four stream operations (there were eight, two of them copies from pageable memory): the sequences go
        // through the pinned staging buffer, ONE kernel packs a (zero padding included) and builds b's profile, the "character outside ACGT"
        // flag is a word of the host-mapped mailbox.
        uint32_t misc[4] = {0, 0, 0, 0};
        bool good = true;
        try {
            ensure_mailbox(0);
            uint8_t* st = static_cast<uint8_t*>(stage(n + m + 64));
            const size_t off_b = (n + 63) & ~size_t(63);
            if (n) std::memcpy(st, a, n);
            if (m) std::memcpy(st + off_b, b, m);
            volatile uint32_t* mb = reinterpret_cast<volatile uint32_t*>(mbox);
            mb[3] = 0;
            __atomic_thread_fence(__ATOMIC_SEQ_CST);
            good = (n == 0 || hip_ok(hipMemcpyAsync(d_a.ptr, st, n, hipMemcpyHostToDevice, s), "H2D a")) &&
                   (m == 0 || hip_ok(hipMemcpyAsync(d_b.ptr, st + off_b, m, hipMemcpyHostToDevice, s), "H2D b")) &&
                   encode_pair_device(d_a.as<uint8_t>(), (int)n, d_codes.as<uint32_t>(), (int)cw, d_b.as<uint8_t>(), (int)m, d_prof.as<uint64_t>(),
                                      reinterpret_cast<uint32_t*>(mbox_dev) + 3, s) &&
                   hip_ok(hipStreamSynchronize(s), "sync");
            misc[3] = mb[3];
        } catch (const engine::EnginePanic&) {
            good = false;
        }
        if (!good) { err = PA_E_HIP; return; }
        if (misc[3]) {
            set_error("sequence contains a base outside ACGT");
            err = PA_E_INVALID_BASE;
            return;
        }
        ok = true;
    }
    ~HipBackend() {
        if (mbox) (void)hipHostFree(mbox);
        h_stage.release();
        if (s) (void)hipStreamDestroy(s);
    }

    I n() const { return (I)a_.size(); }
    I m() const { return (I)b_.size(); }
    const uint8_t* a() const { return a_.data(); }
    const uint8_t* b() const { return b_.data(); }

    void fail(int code) {
        err = code;
        throw engine::EnginePanic(std::string("HIP backend failure: ") + pa_last_error());
    }

    void enable_h_row() {  // blocks.rs:119-123: vec![(0,0); a.len()]
        if (has_h) return;
        if (!d_h.reserve(a_.size() + 64) || !hip_ok(hipMemsetAsync(d_h.ptr, 0, a_.size() + 64, s), "memset h")) fail(PA_E_HIP);
        has_h = true;
    }

    void* stage(size_t bytes) {
        void* p = h_stage.reserve(bytes);
        if (!p) fail(PA_E_HIP);
        return p;
    }

    static constexpr size_t kMboxV = 64;  // offset of the v words inside the mailbox

    void ensure_mailbox(size_t words, size_t extra_bytes = 0) {
        const size_t need = kMboxV + words * 16 + extra_bytes;
        if (need <= mbox_size) return;
        if (mbox) (void)hipHostFree(mbox);
        mbox = nullptr;
        const size_t want = std::max<size_t>(need * 2, 1 << 16);
        void* hp = nullptr;
        void* dp = nullptr;
        if (!hip_ok(hipHostMalloc(&hp, want, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc(mailbox)") ||
            !hip_ok(hipHostGetDevicePointer(&dp, hp, 0), "hipHostGetDevicePointer"))
            fail(PA_E_HIP);
        mbox = (uint8_t*)hp;
        mbox_dev = (uint8_t*)dp;
        mbox_size = want;
        std::memset(mbox, 0, kMboxV);
        if (!d_counter.ptr && (!d_counter.alloc(64) || !hip_ok(hipMemsetAsync(d_counter.ptr, 0, 64, s), "memset counter"))) fail(PA_E_HIP);
    }

    void ensure_granules(size_t ngran) {
        if (ngran <= gran_zeroed) return;
        const size_t want = std::max<size_t>(ngran * 2, 512);
        if (!d_gran.alloc(want * 8) || !hip_ok(hipMemsetAsync(d_gran.ptr, 0, want * 8, s), "memset gran")) fail(PA_E_HIP);
        gran_zeroed = want;
    }

    // PA_ENGINE_NO_FAST_PATH (tests, diagnostics): no mailbox route at all, every rectangle goes through launch_rect's staged route.
    static bool fast_path_off() {
        static const bool off = getenv("PA_ENGINE_NO_FAST_PATH") != nullptr;
        return off;
    }

    // One round trip through the mailbox: the caller puts its v words behind kMboxV, arms the mailbox, launches a kernel that was given
    // `seq` and the device addresses of the three words, and waits for it; the sum and the v words are then the kernel's.
    volatile uint32_t* mbox_words() { return reinterpret_cast<volatile uint32_t*>(mbox); }
    void arm_mailbox() {
        volatile uint32_t* mb = mbox_words();
        mb[1] = 0;  // err
        mb[2] = 0;  // sum
        ++seq;
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
    }
    void wait_mailbox(const char* kernel) {
        const hipError_t launched = hipGetLastError();
        if (launched != hipSuccess) {
            (void)hip_ok(launched, (std::string(kernel) + " launch").c_str());
            fail(PA_E_HIP);
        }
        // spin on the completion word; the kernel's own spins are bounded, so this ends
        uint64_t spins = 0;
        while (__atomic_load_n(reinterpret_cast<uint32_t*>(mbox), __ATOMIC_ACQUIRE) != seq) {
            if ((++spins & 0xFFFFF) == 0 && hipStreamQuery(s) != hipErrorNotReady) {
                // the stream drained (or failed) without the flag: take the slow, certain route
                if (!hip_ok(hipStreamSynchronize(s), "sync")) fail(PA_E_HIP);
                if (__atomic_load_n(reinterpret_cast<uint32_t*>(mbox), __ATOMIC_ACQUIRE) != seq) {
                    set_error("%s finished without signalling completion", kernel);
                    fail(PA_E_INTERNAL);
                }
            }
        }
        const uint32_t err_word = mbox_words()[1];
        if (err_word != PA_ERR_NONE) {
            set_error("device spin timeout (err=%u)", (unsigned)err_word);
            gran_zeroed = 0;  // the hand-off buffer may be dirty
            fail(PA_E_TIMEOUT);
        }
    }
    Cost mailbox_sum() { return (Cost)(int32_t)mbox_words()[2]; }

    // Fast path of one cost-only rectangle: the strips are described by kernel arguments, `v` / sum / err / done live in
    // the host-mapped mailbox, the host spins on `done`.  One API call (the launch) per block.
    // values_host / hbot_host: the traceback's re-fill through the same mailbox -- every column's V and the bottom row's deltas are
    // written by the kernel straight into host-mapped memory behind the v words (no copy command, no stream synchronisation: 81 -> ~40 us per
    // re-filled block of the loop over the drop-in symbol).
    Cost launch_rect_fast(I i0, I i1, size_t w0, size_t w1, V* v, const uint8_t* hin, uint8_t* hout, bool exact, V* values_host = nullptr,
                          int8_t* hbot_host = nullptr) {
        const int n = i1 - i0;
        const size_t w = w1 - w0;
        const size_t S = strips_of(w);
        const size_t G = (size_t)(n + 31) / 32;
        const bool fill = values_host != nullptr;
        const size_t off_values = kMboxV + ((w * 16 + 63) & ~size_t(63)), values_bytes = fill ? (size_t)n * w * 16 : 0;
        const size_t off_hbot = off_values + ((values_bytes + 63) & ~size_t(63));
        ensure_mailbox(w, fill ? (off_hbot - kMboxV - w * 16) + (size_t)n + 64 : 0);
        ensure_granules(S > 1 ? (S - 1) * G : 0);
        std::memcpy(mbox + kMboxV, v, w * 16);
        arm_mailbox();
        RectArgs r;
        r.a_codes = d_codes.as<uint32_t>();
        r.b_prof = d_prof.as<uint32_t>();
        r.v = reinterpret_cast<uint32_t*>(mbox_dev + kMboxV) - w0 * 4;
        r.hin_arr = hin;
        r.hout_arr = fill ? mbox_dev + off_hbot - i0 : hout;  // (indexed by absolute column)
        r.gran = d_gran.as<uint64_t>();
        r.gran_stride = G;
        r.sum_out = reinterpret_cast<int32_t*>(mbox_dev) + 2;
        r.err = reinterpret_cast<uint32_t*>(mbox_dev) + 1;
        r.done = reinterpret_cast<uint32_t*>(mbox_dev);
        r.counter = d_counter.as<uint32_t>();
        r.n = n;
        r.col0 = i0;
        r.w0 = (int)w0;
        r.w1 = (int)w1;
        r.exact_end = exact ? 1 : 0;
        r.seq = seq;
        r.values = fill ? reinterpret_cast<uint32_t*>(mbox_dev + off_values) : nullptr;
        r.fill_stride = (int)w;
        if (fill) hipLaunchKernelGGL((rect_kernel<1, true>), dim3((unsigned)S), dim3(64), 0, s, r);
        else hipLaunchKernelGGL((rect_kernel<1>), dim3((unsigned)S), dim3(64), 0, s, r);
        wait_mailbox("rect_kernel");
        std::memcpy(v, mbox + kMboxV, w * 16);
        if (fill) {
            std::memcpy(values_host, mbox + off_values, values_bytes);
            std::memcpy(hbot_host, mbox + off_hbot, (size_t)n);
        }
        return mailbox_sum();
    }

    // The ranges of one block of the incremental doubling (blocks.rs:370-469) in ONE launch.  Equivalent to calling
    // compute() for every segment in order; the bottom-row sum of the last segment is returned.
    struct ChainSeg {
        size_t w0, w1;
        V* v;
        HMode mode;
    };
    Cost compute_chain(I i0, I i1, const ChainSeg* segs, int nseg, const BlockParams& bp) {
        const I n = i1 - i0;
        bool fuse = !fast_path_off() && n > 0 && nseg >= 2 && nseg <= 3 && has_h;
        size_t strips = 0, lo = SIZE_MAX, hi = 0;
        for (int k = 0; k < nseg && fuse; ++k) {
            if (segs[k].w0 >= segs[k].w1) fuse = false;  // empty ranges have side effects of their own (see compute())
            if (k > 0 && segs[k].w0 < segs[k - 1].w1) fuse = false;
            strips += strips_of(segs[k].w1 - segs[k].w0);
            lo = std::min(lo, segs[k].w0);
            hi = std::max(hi, segs[k].w1);
        }
        if (fuse && strips > 1024) fuse = false;
        if (!fuse) {
            Cost last = 0;
            for (int k = 0; k < nseg; ++k) last = compute(i0, i1, segs[k].w0, segs[k].w1, segs[k].v, segs[k].mode, bp);
            return last;
        }
        const size_t G = (size_t)(n + 31) / 32;
        ensure_mailbox(hi - lo);
        ensure_granules(strips * G);
        for (int k = 0; k < nseg; ++k) std::memcpy(mbox + kMboxV + (segs[k].w0 - lo) * 16, segs[k].v, (segs[k].w1 - segs[k].w0) * 16);
        arm_mailbox();
        ChainArgs r;
        r.a_codes = d_codes.as<uint32_t>();
        r.b_prof = d_prof.as<uint32_t>();
        r.v = reinterpret_cast<uint32_t*>(mbox_dev + kMboxV) - lo * 4;
        r.h_arr = d_h.as<uint8_t>();
        r.gran = d_gran.as<uint64_t>();
        r.gran_stride = G;
        r.sum_out = reinterpret_cast<int32_t*>(mbox_dev) + 2;
        r.err = reinterpret_cast<uint32_t*>(mbox_dev) + 1;
        r.done = reinterpret_cast<uint32_t*>(mbox_dev);
        r.counter = d_counter.as<uint32_t>();
        r.n = n;
        r.col0 = i0;
        r.nseg = nseg;
        r.seq = seq;
        bool prev_stores = false;
        for (int k = 0; k < 3; ++k) {
            r.w0[k] = r.w1[k] = r.top[k] = r.store[k] = 0;
            if (k >= nseg) continue;
            r.w0[k] = (int32_t)segs[k].w0;
            r.w1[k] = (int32_t)segs[k].w1;
            const HMode m = segs[k].mode;
            r.store[k] = (m == HMode::Update || m == HMode::Output) ? 1 : 0;
            if (m == HMode::None || m == HMode::Output) r.top[k] = kTopOne;
            else if (prev_stores && k > 0 && segs[k - 1].w1 == segs[k].w0) r.top[k] = kTopChain;  // the row the segment above stores
            else r.top[k] = kTopStored;
            prev_stores = r.store[k] != 0;
        }
        hipLaunchKernelGGL((rect_chain_kernel<1>), dim3((unsigned)strips), dim3(64), 0, s, r);
        wait_mailbox("rect_chain_kernel");
        for (int k = 0; k < nseg; ++k) std::memcpy(segs[k].v, mbox + kMboxV + (segs[k].w0 - lo) * 16, (segs[k].w1 - segs[k].w0) * 16);
        return mailbox_sum();
    }

    // One rectangle launch.  hin/hout are device byte rows indexed by absolute column (or nullptr).
    // Per call: ONE H2D of a pinned staging image [ticket,err,sum,pad | v words | jobs] into `d_call`, an optional
    // granule clear (only when the rectangle spans several strips), the launch, ONE D2H of [misc | v], one sync.
    Cost launch_rect(I i0, I i1, size_t w0, size_t w1, V* v, const uint8_t* hin, uint8_t* hout, bool exact,
                     V* values_host, int8_t* hbot_host) {
        const int n = i1 - i0;
        const size_t w = w1 - w0;
        const bool fill = values_host != nullptr;
        const size_t S = strips_of(w);
        if (!fill && !fast_path_off() && S <= 1024) return launch_rect_fast(i0, i1, w0, w1, v, hin, hout, exact);
        if (fill && !fast_path_off() && hin == nullptr && (size_t)n * w * 16 <= (size_t(1) << 20) && S <= 64)
            return launch_rect_fast(i0, i1, w0, w1, v, nullptr, nullptr, exact, values_host, hbot_host);
        const size_t ngran = rect_granules(n, (int)w);
        const size_t G = (size_t)(n + 31) / 32;
        ensure_granules(ngran);
        if (fill && d_values.size < (size_t)n * w * 16 && !d_values.alloc((size_t)n * w * 16 * 2)) fail(PA_E_HIP);
        const size_t off_v = 64, off_jobs = off_v + ((w * 16 + 63) & ~size_t(63));
        const size_t total = off_jobs + S * sizeof(StripJob);
        if (d_call.size < total && !d_call.alloc(total * 2)) fail(PA_E_HIP);
        uint8_t* dev = d_call.as<uint8_t>();

        std::vector<StripJob> jobs;
        RectPlan r;
        r.a_codes = d_codes.as<uint32_t>();
        r.col0 = i0;
        r.b_prof = d_prof.as<uint32_t>();
        // the strip indexes v by absolute word: bias the pointer so that word w0 lands at dev + off_v
        r.v = reinterpret_cast<uint32_t*>(dev + off_v) - w0 * 4;
        r.n = n;
        r.w0 = (int)w0;
        r.w1 = (int)w1;
        r.hin_arr = hin;
        r.hout_arr = hout;
        r.gran = d_gran.as<uint64_t>();
        r.gran_stride = G;
        r.sum_out = reinterpret_cast<int32_t*>(dev) + 2;
        r.exact_end = exact;
        r.values = fill ? d_values.as<uint32_t>() : nullptr;
        r.fill_stride = (int)w;
        r.fill_word0 = 0;
        plan_rect(jobs, r);
        if (fill)
            for (auto& j : jobs) j.fill_word0 = j.word0 - (int)w0;

        uint8_t* st = (uint8_t*)stage(total);
        std::memset(st, 0, off_v);
        std::memcpy(st + off_v, v, w * 16);
        std::memcpy(st + off_jobs, jobs.data(), jobs.size() * sizeof(StripJob));
        bool good = hip_ok(hipMemcpyAsync(dev, st, total, hipMemcpyHostToDevice, s), "H2D call image") &&
                    launch_strips(reinterpret_cast<const StripJob*>(dev + off_jobs), (int)jobs.size(), fill,
                                  reinterpret_cast<uint32_t*>(dev), s, /*zero_ticket=*/false) &&
                    hip_ok(hipMemcpyAsync(st, dev, off_v + w * 16, hipMemcpyDeviceToHost, s), "D2H misc+v");
        if (good && fill) {
            good = hip_ok(hipMemcpyAsync(values_host, d_values.ptr, (size_t)n * w * 16, hipMemcpyDeviceToHost, s), "D2H values") &&
                   hip_ok(hipMemcpyAsync(hbot_host, hout + i0, (size_t)n, hipMemcpyDeviceToHost, s), "D2H hbot");
        }
        good = good && hip_ok(hipStreamSynchronize(s), "sync");
        if (!good) fail(PA_E_HIP);
        const uint32_t* misc = reinterpret_cast<const uint32_t*>(st);
        if (misc[1] != PA_ERR_NONE) {
            set_error("device spin timeout (err=%u)", misc[1]);
            fail(PA_E_TIMEOUT);
        }
        std::memcpy(v, st + off_v, w * 16);
        return (Cost)(int32_t)misc[2];
    }

    std::vector<uint8_t> read_h_row(I i0, I i1) {
        std::vector<uint8_t> h((size_t)(i1 - i0));
        if (!hip_ok(hipMemcpyAsync(h.data(), d_h.as<uint8_t>() + i0, h.size(), hipMemcpyDeviceToHost, s), "D2H h") ||
            !hip_ok(hipStreamSynchronize(s), "sync"))
            fail(PA_E_HIP);
        return h;
    }
    Cost sum_h_row(I i0, I i1) {  // empty word range: bottom row == top row
        Cost c = 0;
        for (uint8_t x : read_h_row(i0, i1)) c += h_delta(x);
        return c;
    }

    // blocks.rs:686-748 (the `simd` / `no_ilp` switches select CPU schedules in the reference; results are
    // schedule independent, the GPU always runs its strip schedule).
    Cost compute(I i0, I i1, size_t w0, size_t w1, V* v, HMode mode, const BlockParams&) {
        const I n = i1 - i0;
        if (n <= 0) return 0;
        if (w0 >= w1) {
            switch (mode) {
                case HMode::None: return n;
                case HMode::Output:
                    if (!hip_ok(hipMemsetAsync(d_h.as<uint8_t>() + i0, 1, (size_t)n, s), "memset h")) fail(PA_E_HIP);
                    return n;
                default: return sum_h_row(i0, i1);
            }
        }
        switch (mode) {
            case HMode::None: return launch_rect(i0, i1, w0, w1, v, nullptr, nullptr, false, nullptr, nullptr);
            case HMode::Input: return launch_rect(i0, i1, w0, w1, v, d_h.as<uint8_t>(), nullptr, false, nullptr, nullptr);
            case HMode::Update: return launch_rect(i0, i1, w0, w1, v, d_h.as<uint8_t>(), d_h.as<uint8_t>(), true, nullptr, nullptr);
            case HMode::Output: return launch_rect(i0, i1, w0, w1, v, nullptr, d_h.as<uint8_t>(), true, nullptr, nullptr);
        }
        return 0;
    }

    // blocks.rs:627-648
    void fill(I i0, I i1, size_t w0, size_t w1, V* v, V* values, int8_t* hbot, const BlockParams&) {
        const I n = i1 - i0;
        if (n <= 0) return;
        if (w0 >= w1) {
            for (I i = 0; i < n; ++i) hbot[i] = 1;
            return;
        }
        std::vector<int8_t> raw((size_t)n);
        launch_rect(i0, i1, w0, w1, v, nullptr, d_htmp.as<uint8_t>(), true, values, raw.data());
        for (I i = 0; i < n; ++i) hbot[i] = (int8_t)h_delta((uint8_t)raw[i]);
    }

    std::vector<int8_t> debug_read_h(I i0, I i1) {
        std::vector<int8_t> r;
        for (uint8_t x : read_h_row(i0, i1)) r.push_back((int8_t)h_delta(x));
        return r;
    }
    void debug_write_h(I i0, I i1, const std::vector<int8_t>& x) {
        std::vector<uint8_t> h((size_t)(i1 - i0));
        for (size_t k = 0; k < h.size(); ++k) h[k] = (uint8_t)((x[k] > 0 ? 1 : 0) | (x[k] < 0 ? 2 : 0));
        if (!hip_ok(hipMemcpyAsync(d_h.as<uint8_t>() + i0, h.data(), h.size(), hipMemcpyHostToDevice, s), "H2D h") ||
            !hip_ok(hipStreamSynchronize(s), "sync"))
            fail(PA_E_HIP);
    }
};

// One backend per host thread and device, reused from call to call.
static std::unique_ptr<HipBackend>& pooled_backend_slot() {
    static thread_local std::unique_ptr<HipBackend> tl;
    return tl;
}
static HipBackend& pooled_backend() {
    std::unique_ptr<HipBackend>& tl = pooled_backend_slot();
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!tl || (tl->device >= 0 && tl->device != dev)) tl = std::make_unique<HipBackend>();
    return *tl;
}

}  // namespace pa
