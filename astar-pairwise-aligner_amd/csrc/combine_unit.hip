// combine_unit.hip -- call combining behind pa_align and the astarpa-c symbols: callers inside at the same time become one batch.
// No kernels: it uses the public pa_batch_* entry points and the gathering protocol of combine_logic.hpp.
//
// The reference's entry points are stateless and re-entrant (astarpa-c/src/lib.rs:8-46): a multi-threaded caller aligns one pair per
// thread at a time.  On the GPU one pair at a time is latency bound (a 10 kbp pair: 2 ms through the sweep, whatever else the chip could
// do), while the batch kernels run thousands side by side and return per pair EXACTLY what pa_align returns -- cost, CIGAR string and
// statistics (tests/test_gpu_apa2_batch.py, test_gpu_apa2_full.py, test_gpu_restated_fixtures.py).  So callers that are inside
// pa_align AT THE SAME TIME with the same parameters are combined: a caller that finds nobody gathering gathers -- for 300 us, or until
// everybody who is inside has queued --, aligns the gathered requests as ONE batch (pa_batch_create_params + pa_batch_align) and hands
// the results out; requests that arrive meanwhile are gathered by the next caller, whose batch runs beside the first.  No timer: below a dozen
// concurrent callers (crowd_threshold below) everybody keeps the single-pair path and its latency; above, the batch grows with the number
// of callers by itself.  PA_COMBINE=0 switches it off.
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "combine_logic.hpp"
#include "pa_hip_internal.hpp"

namespace pa {

namespace {
struct CombineReq {
    const uint8_t* a;
    size_t a_len;
    const uint8_t* b;
    size_t b_len;
    int32_t cost = 0;
    std::string cigar;
    pa_astarpa2_stats stats{};
    int rc = 0;
    bool done = false;
    bool queued = false;  // still in the gatherer's pending list (combine_logic.hpp: only such a caller gathers)
    std::string err;
};
struct Combiner {
    pa_astarpa2_params params;  // the key (byte-wise: a parameter set is plain data) ...
    int device = 0;             // ... together with the device the callers are bound to (pa_set_device is per thread): callers on different
                                // GPUs are not mixed, a batch runs on the device of those who asked for it
    combine::Gatherer<CombineReq> g;  // the gathering protocol (combine_logic.hpp; oracle/combine_emu.cpp runs it on host threads under TSan)
};
std::mutex& g_comb_mu = *new std::mutex;
std::vector<Combiner*>& g_combs = *new std::vector<Combiner*>;  // (never destroyed: callers may be inside at exit)
std::atomic<int> g_inside{0};              // eligible callers inside align_hip right now (CombineInside)
std::atomic<uint64_t> g_comb_calls{0}, g_comb_batches{0};
thread_local bool t_in_combiner = false;   // the leader's own batch may hand a pair back to pa_align's engine: that call is not combined again
constexpr int kNotCombined = 1;
// Longer pairs keep the single-pair engine (many wavefronts per pass).  PA_COMBINE_MAX_LEN overrides (experiments).
inline size_t combine_max_len() {
    const char* e = std::getenv("PA_COMBINE_MAX_LEN");
    return e ? (size_t)std::atoll(e) : (size_t)32768;
}
constexpr size_t kCombineMaxGroup = 8192;
constexpr int kCombineInFlight = 8;        // batches of one parameter set on the GPU at a time
constexpr int kCombineWindowUs = 300;      // how long a gathering caller waits for more callers
// Who takes which route.  A batch costs what its slowest pair costs ONE wavefront -- band search and traceback of a 10 kbp pair at 15 %:
// 6-8 ms -- whatever its size, while the single-pair path runs a pair's passes on many wavefronts (2 ms) and eight callers side by side
// reach 1 300-1 400 pairs/s: combining pays from about a dozen concurrent callers on.  And the two routes do not mix: every single-pair
// call keeps several persistent kernels in flight that poll each other, a batch queued behind them waits (measured: 64 threads, eight of
// them on the single-pair path: 875 pairs/s; all combined: 6 000; sixty-four single-pair calls at once starve one another into their
// bounded waits; profiles/r05_runs/dropin_threads.log).  So the library is in one of two modes: as long as fewer than kCrowd callers are
// inside at a time, everybody takes the single-pair path; once kCrowd are, everybody is combined -- and stays so for kSticky after the
// crowd was last seen (the callers of a finished batch leave together and come back one by one: the first ones back must not find the
// place empty and start single-pair calls again).  PA_COMBINE_MIN overrides kCrowd (tests: 2).
std::atomic<int64_t> g_crowded_until{0};  // steady-clock nanoseconds
constexpr int64_t kStickyNs = 20 * 1000 * 1000;
inline int crowd_threshold() {  // (read at every call: tests switch it inside one process)
    const char* e = std::getenv("PA_COMBINE_MIN");
    const int v = e ? std::atoi(e) : 12;
    return v < 2 ? 2 : v;
}
inline bool combine_now() {
    const int64_t now = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    if (g_inside.load(std::memory_order_relaxed) >= crowd_threshold()) {
        g_crowded_until.store(now + kStickyNs, std::memory_order_relaxed);
        return true;
    }
    return now < g_crowded_until.load(std::memory_order_relaxed);
}

Combiner& combiner_for(const pa_astarpa2_params& params) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    // the last combiner this thread used: no global lock, no scan of the (never shrinking) list on the common path
    thread_local Combiner* t_last = nullptr;
    if (t_last && t_last->device == dev && std::memcmp(&t_last->params, &params, sizeof(params)) == 0) return *t_last;
    std::lock_guard<std::mutex> lk(g_comb_mu);
    for (Combiner* c : g_combs)
        if (c->device == dev && std::memcmp(&c->params, &params, sizeof(params)) == 0) return *(t_last = c);
    Combiner* c = new Combiner;
    c->params = params;
    c->device = dev;
    g_combs.push_back(c);
    return *(t_last = c);
}

void run_group(std::vector<CombineReq*>& group, const pa_astarpa2_params& params) {
    const size_t n = group.size();
    std::vector<const uint8_t*> ap(n), bp(n);
    std::vector<size_t> al(n), bl(n);
    for (size_t i = 0; i < n; ++i) {
        ap[i] = group[i]->a;
        bp[i] = group[i]->b;
        al[i] = group[i]->a_len;
        bl[i] = group[i]->b_len;
    }
    std::vector<int32_t> costs(n, 0);
    std::vector<pa_astarpa2_stats> st(n);
    // RAII: a std::string assignment below may throw; the CIGARs the batch malloc'ed and the batch itself go either way,
    // and no request is left half filled (rc is written last, per request, and the caller's catch sets rc_failed for the whole group)
    struct Cigars {
        std::vector<char*> p;
        explicit Cigars(size_t k) : p(k, nullptr) {}
        ~Cigars() {
            for (char* q : p) std::free(q);
        }
    } cigars(n);
    struct InCombiner {
        InCombiner() { t_in_combiner = true; }
        ~InCombiner() { t_in_combiner = false; }
    };
    int rc = 0;
    {
        InCombiner guard;
        std::unique_ptr<pa_batch, void (*)(pa_batch*)> bt(pa_batch_create_params(ap.data(), al.data(), bp.data(), bl.data(), n, &params), pa_batch_destroy);
        if (!bt) rc = kNotCombined;  // (every caller falls back to the single-pair path, which reports its own errors)
        else {
            rc = pa_batch_align(bt.get(), costs.data(), cigars.p.data(), nullptr, nullptr);
            if (rc == 0) rc = pa_batch_pair_stats(bt.get(), st.data());
            if (rc != 0) rc = kNotCombined;
        }
    }
    for (size_t i = 0; i < n; ++i) {
        CombineReq& r = *group[i];
        if (rc == 0) {
            r.cigar = cigars.p[i] ? cigars.p[i] : "";  // (may throw: nothing of r has been touched yet)
            r.cost = costs[i];
            r.stats = st[i];
        }
        r.rc = rc;
    }
    g_comb_calls += n;
    g_comb_batches += 1;
}

}  // namespace

// ---- the interface (pa_hip_internal.hpp) --------------------------------------------------------------------------------------

bool combine_eligible(size_t a_len, size_t b_len, const pa_astarpa2_params& params) {
    return !t_in_combiner && a_len > 0 && b_len > 0 && a_len < combine_max_len() && b_len < combine_max_len() && pa_batch_params_supported(&params);
}

CombineInside::CombineInside() { g_inside.fetch_add(1, std::memory_order_relaxed); }
CombineInside::~CombineInside() { g_inside.fetch_sub(1, std::memory_order_relaxed); }

// 0: done (results filled in); nonzero: the caller runs the single-pair path (combining is off, there is no crowd, or the batch failed).
int combine_align(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, const pa_astarpa2_params& params, int32_t* cost_out,
                  std::string* cigar_out, pa_astarpa2_stats* stats_out) {
    static const bool combine_off = std::getenv("PA_COMBINE") != nullptr && std::getenv("PA_COMBINE")[0] == '0';
    if (combine_off || !combine_now()) return kNotCombined;
    Combiner& c = combiner_for(params);
    CombineReq req{a, a_len, b, b_len};
    // A call lasts as long as its batch, and a batch of short pairs takes about 6 ms whatever its size, so N callers complete N calls per
    // (batch + window): the window is cheap and decides the batch size; several batches run side by side on streams of their own.
    c.g.submit(
        req,
        [&](std::vector<CombineReq*>& group) {
            try {
                run_group(group, params);
            } catch (...) {  // (out of host memory while gathering: every caller of the group takes the single-pair path)
                t_in_combiner = false;
                throw;
            }
        },
        [] { return g_inside.load(std::memory_order_relaxed); }, kCombineMaxGroup, kCombineInFlight, kCombineWindowUs, kNotCombined);
    if (req.rc != 0) return kNotCombined;
    if (cost_out) *cost_out = req.cost;
    if (cigar_out) *cigar_out = std::move(req.cigar);
    if (stats_out) *stats_out = req.stats;
    return 0;
}

// Diagnostics: calls served through the combiner so far, and the batches they went out in.
extern "C" void pa_combine_stats(uint64_t* calls, uint64_t* batches) {
    if (calls) *calls = g_comb_calls.load();
    if (batches) *batches = g_comb_batches.load();
}

}  // namespace pa
