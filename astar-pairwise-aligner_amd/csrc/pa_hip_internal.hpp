// pa_hip_internal.hpp -- shared declarations of the host side of libastarpa_c_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pa_astarpa2.h"
#include "../../include/pa_bitpacking_hip.h"
#include "strip_kernel.hpp"

namespace pa {

constexpr int kWordsPerStrip = 32;  // per subword-per-lane: a strip of k subwords/lane covers 32*k reference words (2048*k rows)

void set_error(const char* fmt, ...);
bool hip_ok(hipError_t e, const char* what);
bool ensure_device();
int device_cus();  // compute units of the device this thread last initialised (ensure_device), 256 if none
// set_error + return rc
int fail(int rc, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// runtime_unit.hip's pools, for the life of the process: pinned host blocks, the chunk streams (non-blocking) and the batches' own
// (blocking) streams; a stream goes back with the device it was created on, after its owner has waited for it
void* pinned_take(size_t bytes, size_t* got);
void pinned_give(void* ptr, size_t size);
hipStream_t stream_take();
void stream_give(hipStream_t s, int dev);
hipStream_t bstream_take();
void bstream_give(hipStream_t s, int dev);

void release_alloc_cache();  // the cached device blocks back to the driver (pa_release_pools)
void release_scope_begin();  // one device wait now; DeviceBuf::release calls of this thread skip theirs until release_scope_end()
void release_scope_end();
void release_scope_begin_waited();  // the caller has waited for everything that used its buffers (its own streams)

struct DeviceBuf {
    void* ptr = nullptr;
    size_t size = 0;
    int device = 0;  // the device ptr lives on
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    ~DeviceBuf() { release(); }
    bool alloc(size_t bytes);
    // grow-only: keeps the buffer when it is large enough; *grew = true when a new (uninitialised) buffer was allocated
    bool reserve(size_t bytes, bool* grew = nullptr);
    void release();
    template <class T>
    T* as() const { return reinterpret_cast<T*>(ptr); }
};
// A pinned host block that only grows (hipHostMallocDefault): a request beyond its size frees it and allocates max(2 * bytes, 64 KiB).
// Its owner keeps it for its own life; it is not one of pinned_take's pooled blocks.
struct PinnedBuf {
    void* ptr = nullptr;
    size_t size = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    void* reserve(size_t bytes) {  // nullptr (and the error set) when the allocation fails
        if (bytes > size) {
            release();
            const size_t want = bytes * 2 > (size_t(1) << 16) ? bytes * 2 : size_t(1) << 16;
            if (!hip_ok(hipHostMalloc(&ptr, want, hipHostMallocDefault), "hipHostMalloc")) return nullptr;
            size = want;
        }
        return ptr;
    }
    void release() {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        size = 0;
    }
};
// d.alloc(max(bytes, 16)), then the copy queued on s
bool upload(DeviceBuf& d, const void* src, size_t bytes, hipStream_t s);
// Device-memory budget of one traced chunk: the megabytes in the environment variable `env_mb`, else a quarter of the free memory.
size_t trace_budget(const char* env_mb);
// A malloc'ed copy of every text into out[0 .. texts.size()).  If one malloc fails, the copies made so far are freed and nulled again
// (the caller owns outputs only on success): "out of memory", PA_E_NOMEM.
int give_cstrings(const std::vector<std::string>& texts, char** out);

// One rectangle = words [w0,w1) x n columns of one pair, split into chained strips.
struct RectPlan {
    const uint32_t* a_codes = nullptr;  // device, packed codes of the whole sequence
    int col0 = 0;                       // absolute first column of the rectangle
    const uint32_t* b_prof = nullptr;   // device, u32 view of the pair's profile (word 0)
    uint32_t* v = nullptr;              // device, u32 view of the v column (word 0 of the same indexing as b_prof)
    int n = 0, w0 = 0, w1 = 0;
    const uint8_t* hin_arr = nullptr;   // per-absolute-column top deltas or nullptr (+1)
    uint8_t* hout_arr = nullptr;        // per-absolute-column bottom deltas out or nullptr
    uint64_t* gran = nullptr;           // (S-1) * gran_stride granules, zeroed before launch
    size_t gran_stride = 0;             // >= ceil(n/16)
    int32_t* sum_out = nullptr;
    bool exact_end = false;
    bool v_init_one = false;
    int tail_rows = -1;  // see StripJob::tail_rows
    uint32_t* values = nullptr;  // fill mode
    int fill_stride = 0, fill_word0 = 0;
    bool pingpong = false;  // sequential-pairs mode: two granule rows per rectangle, strip s writes row s&1;
                            // the ragged bottom is planned as short k = 1 strips (strip_plan)
    int k = 1;  // 32-row subwords per lane (1: lowest latency; 2, 4: fewer instructions per cell, cost-only strips)
    uint32_t* ckpt = nullptr;  // traced batches: V column after every 256th column (StripJob::ckpt)
    int ckpt_stride = 0;
};

void plan_rect(std::vector<StripJob>& jobs, const RectPlan& r);
// Strips of a rectangle of w words: `full` strips of 32*k words, then `tail1` strips of up to 32 words (sequential mode only).
struct StripPlan {
    int full = 0, tail1 = 0;
    int strips() const { return full + tail1; }
};
StripPlan strip_plan(int w, int k, bool sequential);
size_t rect_granules(int n, int w, int k = 1, bool pingpong = false);
bool launch_strips(const StripJob* d_jobs, int njobs, bool fill, uint32_t* d_ticket_err, hipStream_t s, bool zero_ticket = true,
                   bool scatter = false, int k = 1, int block_waves = kStripBlockWaves, bool ckpt = false);
bool launch_pairs(const StripJob* d_jobs, const int32_t* d_first, int npairs, uint32_t* d_ticket_err, hipStream_t s, int k, bool ckpt = false);
int align_hip(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, const pa_astarpa2_params& params, bool trace, bool self_check,
              int32_t* cost_out, std::string* cigar_out, pa_astarpa2_stats* stats_out);
// combine_unit.hip -- callers inside align_hip at the same time become one batch.  A caller that combine_eligible() accepts (lengths, a
// parameter set the batch kernels take, not the combiner's own batch handing a pair back) holds a CombineInside while it is inside:
// these are the crowd that combine_align() looks at when it decides whether to combine now.  combine_align: 0 = done, results handed
// out; nonzero = not combined, the caller takes the single-pair path.
bool combine_eligible(size_t a_len, size_t b_len, const pa_astarpa2_params& params);
struct CombineInside {
    CombineInside();
    ~CombineInside();
    CombineInside(const CombineInside&) = delete;
    CombineInside& operator=(const CombineInside&) = delete;
};
int combine_align(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, const pa_astarpa2_params& params, int32_t* cost_out,
                  std::string* cigar_out, pa_astarpa2_stats* stats_out);
// The semi-global search's ScatterProfile of a pattern (four u64 match masks per 64-row word, padding rows match everything) and its
// left column v0 (V words), max(ceil(plen / 64), 1) words each.  PA_E_INVALID_BASE on a character outside ACGTNYR* (either case).
int search_profile(const uint8_t* pattern, size_t plen, float unmatched_cost, std::vector<uint64_t>& prof, std::vector<uint64_t>& v0);
bool encode_a_device(const uint8_t* d_a, int n, uint32_t* d_codes, uint32_t* d_bad, hipStream_t s);
bool build_b_device(const uint8_t* d_b, int m, uint64_t* d_prof, uint32_t* d_bad, hipStream_t s);
// both in one launch; all `code_words` words of d_codes are written (zero beyond the sequence); `bad` may be host-mapped memory
bool encode_pair_device(const uint8_t* d_a, int n, uint32_t* d_codes, int code_words, const uint8_t* d_b, int m, uint64_t* d_prof, uint32_t* bad,
                        hipStream_t s);
// Batched forms (all pairs of a pa_batch): where each pair's sequences, codes and profile lie in the concatenated buffers.
// rank in "ACGT" (bio RankTransform as used by BitProfile::build, profile.rs:113); -1 otherwise.  Shared by the encode kernels
// (rect_unit.hip) and the bit-sliced batch's transposes (slice_kernel.hpp), which read the sequences themselves.
__device__ __forceinline__ int rank_acgt(uint8_t c) {
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}

struct PairDesc {
    unsigned long long a_off, b_off, code_off, prof_off;  // element offsets into the concatenated buffers
    int n, m;
};
// codes of every a (skipped when max_n == 0) and profile of every b (skipped when max_m == 0) of `pairs` descriptors
bool encode_batch_device(const uint8_t* d_a_cat, size_t max_n, uint32_t* d_codes_cat, const uint8_t* d_b_cat, size_t max_m, uint64_t* d_prof_cat,
                         const PairDesc* d_desc, size_t pairs, uint32_t* d_bad, hipStream_t s);
// apa2_jobs_unit.hip -- host threads for per-pair host work of a batch (PA_HOST_THREADS, else as many as the process may run on), and
// the words per slot of a pair's block-column store in the batched A*PA2 modes (PA_APA2_WINDOW; override_ < 0: the policy)
unsigned host_threads();
size_t window_words(size_t n, size_t m, bool gcsh, int override_);

}  // namespace pa
