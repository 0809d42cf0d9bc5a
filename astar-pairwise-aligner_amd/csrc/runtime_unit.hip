// runtime_unit.hip -- what every entry point of libastarpa_c_hip.so stands on: the thread's error text, the device context, the cache
// of device blocks behind DeviceBuf, the pools of pinned buffers and streams, the release scopes, and the small host helpers the
// units share.  No kernels.
#include "pa_hip_internal.hpp"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace pa {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    set_error("HIP error in %s: %s", what, hipGetErrorString(e));
    return false;
}

// ---- device context -----------------------------------------------------------------------------

static thread_local int g_device_props_cus = 0;  // of the device this thread last initialised (pa_set_device is per thread)
static thread_local int g_device_props_dev = -1;

bool ensure_device() {
    static thread_local bool inited = false;
    if (inited) {
        int cur = 0;
        if (hipGetDevice(&cur) == hipSuccess && cur == g_device_props_dev) return true;
    }
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) {
        set_error("no HIP device available: the MI355X path is required (there is no CPU fallback)");
        return false;
    }
    int dev = 0;
    if (!hip_ok(hipGetDevice(&dev), "hipGetDevice")) return false;
    hipDeviceProp_t prop;
    if (!hip_ok(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties")) return false;
    g_device_props_cus = prop.multiProcessorCount;
    g_device_props_dev = dev;
    inited = true;
    return true;
}

int device_cus() { return g_device_props_cus > 0 ? g_device_props_cus : 256; }

// ---- device memory -----------------------------------------------------------------------------------------------------------
// Large buffers are CACHED: hipMalloc + hipFree of the 40 GB block-column store of a 4096 x 100 kbp batch cost about a second, seven
// times the alignment of the pairs it holds, and pa_align_file / the work queue create a batch per chunk.  A buffer of at least
// kCacheMin bytes goes to a free list when its owner lets go of it and is handed to the next request on the same device that it fits
// (at most a quarter larger than asked for).  Nothing in this library reads device memory it has not written, and a cached block is
// as undefined as a fresh one.  The list is bounded per device (cache_limit, oldest out first), emptied when an allocation fails, and
// returned to the driver by pa_release_pools().  PA_NO_ALLOC_CACHE=1 switches it off; PA_POISON_ALLOC=1 fills every buffer handed
// out with 0xA5 (tests: nothing may depend on fresh memory being zero).
namespace {
constexpr size_t kCacheMin = size_t(16) << 20, kCacheMaxDefault = size_t(16) << 30;
// The bound is PER DEVICE: PA_ALLOC_CACHE_MAX (bytes, or with a K / M / G suffix) if set, else half of the device's memory, at most 16 GB
// (round 4: with band-proportional block columns a 4096 x 100 kbp A*PA2 batch holds 5 GB, not 40)
// -- other users of the device in the same process (torch, RCCL) cannot make this library let go of what it caches.
size_t cache_limit(int dev) {
    static std::mutex mu;
    static std::vector<size_t> lim;
    std::lock_guard<std::mutex> lk(mu);
    if ((size_t)dev < lim.size() && lim[(size_t)dev]) return lim[(size_t)dev];
    size_t v = 0;
    if (const char* e = getenv("PA_ALLOC_CACHE_MAX")) {
        char* end = nullptr;
        double x = std::strtod(e, &end);
        if (end && (*end == 'G' || *end == 'g')) x *= double(size_t(1) << 30);
        else if (end && (*end == 'M' || *end == 'm')) x *= double(size_t(1) << 20);
        else if (end && (*end == 'K' || *end == 'k')) x *= 1024.0;
        v = x > 0 ? (size_t)x : 1;
    } else {
        size_t free_b = 0, total_b = 0;
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = 0;
        if (cur != dev) (void)hipSetDevice(cur);
        v = total_b ? std::min(kCacheMaxDefault, total_b / 2) : kCacheMaxDefault;
    }
    if ((size_t)dev >= lim.size()) lim.resize((size_t)dev + 1, 0);
    lim[(size_t)dev] = v;
    return v;
}
struct CachedBlock {
    int dev;
    void* ptr;
    size_t size;
};
// (never destroyed: buffers of thread-local pools are released after the statics of this file at process exit)
std::mutex& g_cache_mu = *new std::mutex;
std::vector<CachedBlock>& g_cache = *new std::vector<CachedBlock>;  // oldest first
size_t g_cache_bytes = 0;
std::atomic<uint64_t> g_cache_hits{0}, g_cache_misses{0};

bool cache_on() {
    static const bool off = getenv("PA_NO_ALLOC_CACHE") != nullptr;
    return !off;
}
void* cache_take(int dev, size_t bytes, size_t* got) {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    size_t best = g_cache.size();
    for (size_t i = 0; i < g_cache.size(); ++i)
        if (g_cache[i].dev == dev && g_cache[i].size >= bytes && g_cache[i].size <= bytes + bytes / 4 &&
            (best == g_cache.size() || g_cache[i].size < g_cache[best].size))
            best = i;
    if (best == g_cache.size()) return nullptr;
    void* p = g_cache[best].ptr;
    *got = g_cache[best].size;
    g_cache_bytes -= g_cache[best].size;
    g_cache.erase(g_cache.begin() + (long)best);
    return p;
}
// -> blocks the caller has to hipFree (outside the lock)
std::vector<CachedBlock> cache_put(int dev, void* ptr, size_t size) {
    std::vector<CachedBlock> out;
    const size_t limit = cache_limit(dev);
    std::lock_guard<std::mutex> lk(g_cache_mu);
    g_cache.push_back({dev, ptr, size});
    g_cache_bytes += size;
    size_t on_dev = 0;
    for (const CachedBlock& b : g_cache)
        if (b.dev == dev) on_dev += b.size;
    for (size_t i = 0; i < g_cache.size() && on_dev > limit;) {  // this device's oldest blocks go first
        if (g_cache[i].dev != dev) {
            ++i;
            continue;
        }
        out.push_back(g_cache[i]);
        g_cache_bytes -= g_cache[i].size;
        on_dev -= g_cache[i].size;
        g_cache.erase(g_cache.begin() + (long)i);
    }
    return out;
}
void free_blocks(const std::vector<CachedBlock>& blocks) {
    if (blocks.empty()) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const CachedBlock& b : blocks) {
        if (b.dev != cur) (void)hipSetDevice(b.dev);
        (void)hipFree(b.ptr);
        if (b.dev != cur) (void)hipSetDevice(cur);
    }
}
}  // namespace

// PA_POISON_ALLOC: on a stream of its own that does not synchronise with the null stream (persistent kernels may be in flight)
static bool poison_fill(void* ptr, size_t size) {
    static thread_local hipStream_t st = nullptr;
    if (!st && !hip_ok(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "poison stream")) return false;
    return hip_ok(hipMemsetAsync(ptr, 0xA5, size, st), "poison") && hip_ok(hipStreamSynchronize(st), "poison sync");
}

void pinned_release_all();
void release_alloc_cache() {
    pinned_release_all();
    std::vector<CachedBlock> all;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        all.swap(g_cache);
        g_cache_bytes = 0;
    }
    free_blocks(all);
}

extern "C" void pa_alloc_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* cached_bytes) {
    if (hits) *hits = g_cache_hits.load();
    if (misses) *misses = g_cache_misses.load();
    if (cached_bytes) {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        *cached_bytes = g_cache_bytes;
    }
}

bool DeviceBuf::alloc(size_t bytes) {
    release();
    if (bytes < 64) bytes = 64;
    static const bool poison = getenv("PA_POISON_ALLOC") != nullptr;
    int dev = 0;
    if (!hip_ok(hipGetDevice(&dev), "hipGetDevice")) return false;
    // Small buffers are cached too (round 5), in size classes (2^k and 1.5 x 2^k): a batch of a few pairs -- what the call combiner behind
    // pa_align creates a thousand times a second -- made some thirty hipMalloc / hipFree calls of 50-100 us each, every hipFree a device wait.
    const bool big = cache_on();
    if (big && bytes < kCacheMin) {
        size_t c = 64;
        while (c < bytes) c = (c + c / 2 >= bytes && (c & (c - 1)) == 0) ? c + c / 2 : ((c & (c - 1)) == 0 ? c * 2 : (c / 3) * 4);
        bytes = c;
    }
    if (big) {
        if (bytes >= kCacheMin) bytes = (bytes + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);  // (2 MB steps: requests of almost the same size meet)
        size_t got = 0;
        if (void* p = cache_take(dev, bytes, &got)) {
            ptr = p;
            size = got;
            device = dev;
            g_cache_hits += 1;
            if (poison && !poison_fill(ptr, size)) return false;
            return true;
        }
        g_cache_misses += 1;
    }
    hipError_t e = hipMalloc(&ptr, bytes);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {  // give the cached blocks back and try once more
        (void)hipGetLastError();
        release_alloc_cache();
        e = hipMalloc(&ptr, bytes);
    }
    if (!hip_ok(e, "hipMalloc")) {
        ptr = nullptr;
        return false;
    }
    size = bytes;
    device = dev;
    if (poison && !poison_fill(ptr, size)) return false;
    return true;
}
bool DeviceBuf::reserve(size_t bytes, bool* grew) {
    if (grew) *grew = false;
    if (ptr && size >= bytes) return true;
    const size_t want = bytes + bytes / 4 + 256;  // geometric growth: a pool of buffers reused from call to call
    if (!alloc(want)) return false;
    if (grew) *grew = true;
    return true;
}
// Pinned host buffers (the packed CIGAR text of a batch, its per-pair lengths) are POOLED for the life of the process: hipHostMalloc /
// hipHostFree of a few tens of megabytes cost 5-25 ms each, which a batch that lives for one alignment (the work queue's chunks, pa_align_file)
// paid twice (round 4: `close` of the C4 batch 12-50 ms).  At most kPinnedPoolMax bytes are kept; pa_release_pools() frees them.
namespace {
constexpr size_t kPinnedPoolMax = size_t(1) << 30;
struct PinnedBlock {
    void* ptr;
    size_t size;
};
std::mutex& g_pin_mu = *new std::mutex;
std::vector<PinnedBlock>& g_pin = *new std::vector<PinnedBlock>;
size_t g_pin_bytes = 0;
}  // namespace
void* pinned_take(size_t bytes, size_t* got) {
    {  // size classes (2^k and 1.5 x 2^k from 64 KB up): batches of slightly different sizes -- the call combiner's -- meet in the pool
        size_t c = size_t(64) << 10;
        while (c < bytes) c = ((c & (c - 1)) == 0 && c + c / 2 >= bytes) ? c + c / 2 : ((c & (c - 1)) == 0 ? c * 2 : (c / 3) * 4);
        bytes = c;
    }
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        size_t best = g_pin.size();
        for (size_t i = 0; i < g_pin.size(); ++i)
            // (best fit, and never a block more than twice the request + 64 KB: a 100 KB request must not take the pooled 30 MB text
            //  buffer and send the next text request back to hipHostMalloc)
            if (g_pin[i].size >= bytes && g_pin[i].size <= 2 * bytes + 65536 && (best == g_pin.size() || g_pin[i].size < g_pin[best].size)) best = i;
        if (best != g_pin.size()) {
            void* p = g_pin[best].ptr;
            *got = g_pin[best].size;
            g_pin_bytes -= g_pin[best].size;
            g_pin.erase(g_pin.begin() + (long)best);
            return p;
        }
    }
    void* hp = nullptr;
    if (!hip_ok(hipHostMalloc(&hp, bytes, hipHostMallocDefault), "hipHostMalloc(pinned pool)")) return nullptr;
    *got = bytes;
    return hp;
}
void pinned_give(void* ptr, size_t size) {
    if (!ptr) return;
    std::vector<PinnedBlock> drop;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        g_pin.push_back({ptr, size});
        g_pin_bytes += size;
        while (g_pin_bytes > kPinnedPoolMax && !g_pin.empty()) {
            drop.push_back(g_pin.front());
            g_pin_bytes -= g_pin.front().size;
            g_pin.erase(g_pin.begin());
        }
    }
    for (const PinnedBlock& b : drop) (void)hipHostFree(b.ptr);
}
// ... and so are the chunk streams of pa_batch_align (hipStreamDestroy costs ~3 ms each: a C4 batch of four chunks spent 12 ms of its
// `close` there); per device, idle when they are handed back (the batch's destructor has waited for the device).
namespace {
std::vector<std::pair<int, hipStream_t>>& g_streams = *new std::vector<std::pair<int, hipStream_t>>;
}
hipStream_t stream_take() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        for (size_t i = 0; i < g_streams.size(); ++i)
            if (g_streams[i].first == dev) {
                hipStream_t s = g_streams[i].second;
                g_streams.erase(g_streams.begin() + (long)i);
                return s;
            }
    }
    hipStream_t s = nullptr;
    if (!hip_ok(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate")) return nullptr;
    return s;
}
// The batch's own stream (a default, blocking stream: its work orders with the synchronous copies of the creation) is pooled as well:
// hipStreamCreate costs 2 ms, a quarter of what a batch of sixteen short pairs takes from creation to destruction (round 5: the call
// combiner behind pa_align creates such batches a hundred times a second).  A stream goes back only after its batch has waited for the device.
namespace {
std::vector<std::pair<int, hipStream_t>>& g_bstreams = *new std::vector<std::pair<int, hipStream_t>>;
}
hipStream_t bstream_take() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        for (size_t i = 0; i < g_bstreams.size(); ++i)
            if (g_bstreams[i].first == dev) {
                hipStream_t s = g_bstreams[i].second;
                g_bstreams.erase(g_bstreams.begin() + (long)i);
                return s;
            }
    }
    hipStream_t s = nullptr;
    if (!hip_ok(hipStreamCreate(&s), "hipStreamCreate")) return nullptr;
    return s;
}
void bstream_give(hipStream_t s, int dev) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        if (g_bstreams.size() < 32) {
            g_bstreams.emplace_back(dev, s);
            return;
        }
    }
    (void)hipStreamDestroy(s);
}
void stream_give(hipStream_t s, int dev) {  // dev: the device the stream was created on (a batch may be destroyed from a thread bound to another)
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        if (g_streams.size() < 64) {
            g_streams.emplace_back(dev, s);
            return;
        }
    }
    (void)hipStreamDestroy(s);
}
void pinned_release_all() {
    {
        std::vector<std::pair<int, hipStream_t>> st;
        {
            std::lock_guard<std::mutex> lk(g_pin_mu);
            st.swap(g_streams);
        }
        for (auto& x : st) (void)hipStreamDestroy(x.second);
    }
    std::vector<PinnedBlock> all;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        all.swap(g_pin);
        g_pin_bytes = 0;
    }
    for (const PinnedBlock& b : all) (void)hipHostFree(b.ptr);
}

// A batch lets go of a dozen buffers at once: its destructor waits for the device ONCE and the releases that follow skip their wait.
static thread_local bool g_release_synced = false;
void release_scope_begin() {
    (void)hipDeviceSynchronize();
    g_release_synced = true;
}
// ... or the owner waited for everything that ever touched its buffers itself (a batch: its own streams) and only declares the scope:
// a device-wide wait also waits for every OTHER batch in flight -- eight batches of the call combiner side by side each waited for the
// other seven's kernels (round 5: 40 ms per call at 64 callers instead of 8)
void release_scope_begin_waited() { g_release_synced = true; }
void release_scope_end() { g_release_synced = false; }

void DeviceBuf::release() {
    if (ptr) {
        if (cache_on() && g_release_synced) {  // (inside a release scope the device has been waited for: any size goes to the cache)
            int cur = device;
            (void)hipGetDevice(&cur);
            if (cur == device) {
                free_blocks(cache_put(device, ptr, size));
                ptr = nullptr;
                size = 0;
                return;
            }
        }
        if (size >= kCacheMin && cache_on()) {
            // hipFree waits for the device before it lets a buffer go; a cached block may be handed to another thread at once, so
            // this waits too (whoever must not wait -- the sweep's pool while passes are in flight -- never frees, sweep_hip.hpp)
            int cur = device;
            (void)hipGetDevice(&cur);
            if (cur != device) (void)hipSetDevice(device);  // (a batch destroyed from a thread bound to another GPU)
            (void)hipDeviceSynchronize();
            if (cur != device) (void)hipSetDevice(cur);
            free_blocks(cache_put(device, ptr, size));
        } else {
            (void)hipFree(ptr);
        }
    }
    ptr = nullptr;
    size = 0;
}

// ---- helpers the units share -------------------------------------------------------------------

int fail(int rc, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    set_error("%s", buf);
    return rc;
}

bool upload(DeviceBuf& d, const void* src, size_t bytes, hipStream_t s) {
    if (!d.alloc(std::max<size_t>(bytes, 16))) return false;
    return bytes == 0 || hip_ok(hipMemcpyAsync(d.ptr, src, bytes, hipMemcpyHostToDevice, s), "H2D");
}

size_t trace_budget(const char* env_mb) {
    if (const char* e = getenv(env_mb)) {
        const double mb = atof(e);
        if (mb > 0) return (size_t)(mb * 1048576.0);
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b == 0) return size_t(1) << 30;
    return free_b / 4;
}

int give_cstrings(const std::vector<std::string>& texts, char** out) {
    for (size_t i = 0; i < texts.size(); ++i) {
        out[i] = (char*)std::malloc(texts[i].size() + 1);
        if (!out[i]) {
            for (size_t k = 0; k < i; ++k) {
                std::free(out[k]);
                out[k] = nullptr;
            }
            return fail(PA_E_NOMEM, "out of memory");
        }
        std::memcpy(out[i], texts[i].c_str(), texts[i].size() + 1);
    }
    return 0;
}

}  // namespace pa

using namespace pa;

extern "C" const char* pa_last_error(void) { return g_last_error.c_str(); }

extern "C" int pa_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

extern "C" int pa_set_device(int device) {
    if (!hip_ok(hipSetDevice(device), "hipSetDevice")) return PA_E_HIP;
    return 0;
}
