// rect_unit.hip -- the rectangle operator (include/pa_bitpacking_hip.h): profile kernels, the strip and pair kernels' instances,
// how a rectangle is cut into strips and launched, and pa_bp_profile_build / pa_bp_compute / pa_bp_fill.  gfx950 only.
#include "pa_hip_internal.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace pa {

// ---- device kernels: profile building ---------------------------------------------------------

// One thread per 16 columns: ASCII -> packed 2-bit codes.
__global__ void encode_a_kernel(const uint8_t* __restrict__ a, int n, uint32_t* __restrict__ codes, int nwords,
                                uint32_t* __restrict__ bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwords) return;
    uint32_t w = 0;
    bool invalid = false;
    for (int k = 0; k < 16; ++k) {
        const int c = i * 16 + k;
        if (c < n) {
            const int r = rank_acgt(a[c]);
            invalid |= r < 0;
            w |= (uint32_t)(r & 3) << (2 * k);
        }
    }
    codes[i] = w;
    if (invalid) atomicOr(bad, 1u);
}

// One wave per 64-row word: negated bit-planes via ballot; rows >= m stay (0,0) (profile.rs:127-132).
__global__ void build_b_kernel(const uint8_t* __restrict__ b, int m, uint64_t* __restrict__ prof, int nwords,
                               uint32_t* __restrict__ bad) {
    const int word = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (word >= nwords) return;
    const int lane = threadIdx.x & 63;
    const int j = word * 64 + lane;
    int r = 3;  // (r&1)^1 == 0 and ((r>>1)&1)^1 == 0 => pad rows contribute 0 bits
    bool invalid = false;
    if (j < m) {
        r = rank_acgt(b[j]);
        invalid = r < 0;
        r &= 3;
    }
    const uint64_t nb0 = __ballot(((r & 1) ^ 1) != 0);
    const uint64_t nb1 = __ballot((((r >> 1) & 1) ^ 1) != 0);
    if (lane == 0) {
        prof[2 * word] = nb0;
        prof[2 * word + 1] = nb1;
    }
    if (invalid) atomicOr(bad, 1u);
}

// Batched forms (one launch for all pairs of a pa_batch): blockIdx.y = pair.
__global__ void encode_a_batch_kernel(const uint8_t* __restrict__ a_cat, uint32_t* __restrict__ codes_cat,
                                      const PairDesc* __restrict__ desc, uint32_t* __restrict__ bad) {
    const PairDesc d = desc[blockIdx.y];
    const int nwords = (d.n + 15) / 16;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwords) return;
    const uint8_t* a = a_cat + d.a_off;
    uint32_t w = 0;
    bool invalid = false;
    for (int k = 0; k < 16; ++k) {
        const int c = i * 16 + k;
        if (c < d.n) {
            const int r = rank_acgt(a[c]);
            invalid |= r < 0;
            w |= (uint32_t)(r & 3) << (2 * k);
        }
    }
    codes_cat[d.code_off + i] = w;
    if (invalid) atomicOr(bad, 1u);
}

__global__ void build_b_batch_kernel(const uint8_t* __restrict__ b_cat, uint64_t* __restrict__ prof_cat,
                                     const PairDesc* __restrict__ desc, uint32_t* __restrict__ bad) {
    const PairDesc d = desc[blockIdx.y];
    const int nwords = (d.m + 63) / 64;
    const int word = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (word >= nwords) return;
    const uint8_t* b = b_cat + d.b_off;
    const int lane = threadIdx.x & 63;
    const int j = word * 64 + lane;
    int r = 3;
    bool invalid = false;
    if (j < d.m) {
        r = rank_acgt(b[j]);
        invalid = r < 0;
        r &= 3;
    }
    const uint64_t nb0 = __ballot(((r & 1) ^ 1) != 0);
    const uint64_t nb1 = __ballot((((r >> 1) & 1) ^ 1) != 0);
    if (lane == 0) {
        prof_cat[2 * (d.prof_off + word)] = nb0;
        prof_cat[2 * (d.prof_off + word) + 1] = nb1;
    }
    if (invalid) atomicOr(bad, 1u);
}

template __global__ void strip_kernel<1, false, false>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<1, true, false>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<1, false, true>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<1, true, true>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<2, false, false>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<4, false, false>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<8, false, false>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<1, false, false, true>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<2, false, false, true>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<4, false, false, true>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void strip_kernel<8, false, false, true>(const StripJob*, int, uint32_t*, uint32_t*);
template __global__ void pair_kernel<1>(const StripJob*, const int32_t*, int, uint32_t*);
template __global__ void pair_kernel<2>(const StripJob*, const int32_t*, int, uint32_t*);
template __global__ void pair_kernel<4>(const StripJob*, const int32_t*, int, uint32_t*);
template __global__ void pair_kernel<8>(const StripJob*, const int32_t*, int, uint32_t*);
template __global__ void pair_kernel<1, true>(const StripJob*, const int32_t*, int, uint32_t*);
template __global__ void pair_kernel<2, true>(const StripJob*, const int32_t*, int, uint32_t*);
template __global__ void pair_kernel<4, true>(const StripJob*, const int32_t*, int, uint32_t*);
template __global__ void pair_kernel<8, true>(const StripJob*, const int32_t*, int, uint32_t*);

// Both encodings of ONE pair in one launch (the single-pair engine's per-call set-up, round 6: eight stream operations were four): the
// first blocks pack a -- every word of `codes` up to code_words, so the padding the kernels read past the last column is zeroed here --,
// the others build b's profile.  `bad` may be host-mapped: every writer stores the same 1.
__global__ void encode_pair_kernel(const uint8_t* __restrict__ a, int n, uint32_t* __restrict__ codes, int code_words, int a_blocks,
                                   const uint8_t* __restrict__ b, int m, uint64_t* __restrict__ prof, int prof_words, uint32_t* bad) {
    if ((int)blockIdx.x < a_blocks) {
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= code_words) return;
        uint32_t w = 0;
        bool invalid = false;
        for (int k = 0; k < 16; ++k) {
            const int c = i * 16 + k;
            if (c < n) {
                const int r = rank_acgt(a[c]);
                invalid |= r < 0;
                w |= (uint32_t)(r & 3) << (2 * k);
            }
        }
        codes[i] = w;
        if (invalid) __hip_atomic_store(bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int word = ((int)blockIdx.x - a_blocks) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (word >= prof_words) return;
    const int lane = threadIdx.x & 63;
    const int j = word * 64 + lane;
    int r = 3;
    bool invalid = false;
    if (j < m) {
        r = rank_acgt(b[j]);
        invalid = r < 0;
        r &= 3;
    }
    const uint64_t nb0 = __ballot(((r & 1) ^ 1) != 0);
    const uint64_t nb1 = __ballot((((r >> 1) & 1) ^ 1) != 0);
    if (lane == 0) {
        prof[2 * word] = nb0;
        prof[2 * word + 1] = nb1;
    }
    if (invalid) __hip_atomic_store(bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
bool encode_pair_device(const uint8_t* d_a, int n, uint32_t* d_codes, int code_words, const uint8_t* d_b, int m, uint64_t* d_prof, uint32_t* bad,
                        hipStream_t s) {
    const int a_blocks = (code_words + 255) / 256, prof_words = (m + 63) / 64, b_blocks = (prof_words + 3) / 4;
    if (a_blocks + b_blocks == 0) return true;
    hipLaunchKernelGGL(encode_pair_kernel, dim3((unsigned)(a_blocks + b_blocks)), dim3(256), 0, s, d_a, n, d_codes, code_words, a_blocks, d_b, m, d_prof,
                       prof_words, bad);
    return hip_ok(hipGetLastError(), "encode_pair_kernel");
}

bool encode_a_device(const uint8_t* d_a, int n, uint32_t* d_codes, uint32_t* d_bad, hipStream_t s) {
    const int nwords = (n + 15) / 16;
    if (nwords == 0) return true;
    hipLaunchKernelGGL(encode_a_kernel, dim3((nwords + 255) / 256), dim3(256), 0, s, d_a, n, d_codes, nwords, d_bad);
    return hip_ok(hipGetLastError(), "encode_a_kernel");
}

bool build_b_device(const uint8_t* d_b, int m, uint64_t* d_prof, uint32_t* d_bad, hipStream_t s) {
    const int nwords = (m + 63) / 64;
    if (nwords == 0) return true;
    hipLaunchKernelGGL(build_b_kernel, dim3((nwords + 3) / 4), dim3(256), 0, s, d_b, m, d_prof, nwords, d_bad);
    return hip_ok(hipGetLastError(), "build_b_kernel");
}

bool encode_batch_device(const uint8_t* d_a_cat, size_t max_n, uint32_t* d_codes_cat, const uint8_t* d_b_cat, size_t max_m, uint64_t* d_prof_cat,
                         const PairDesc* d_desc, size_t pairs, uint32_t* d_bad, hipStream_t s) {
    for (size_t base = 0; base < pairs; base += 32768) {  // gridDim.y limit
        const unsigned ny = (unsigned)std::min<size_t>(32768, pairs - base);
        const PairDesc* dd = d_desc + base;
        if (max_n) {
            const unsigned nx = (unsigned)(((max_n + 15) / 16 + 255) / 256);
            hipLaunchKernelGGL(encode_a_batch_kernel, dim3(nx, ny), dim3(256), 0, s, d_a_cat, d_codes_cat, dd, d_bad);
        }
        if (max_m) {
            const unsigned nx = (unsigned)(((max_m + 63) / 64 + 3) / 4);
            hipLaunchKernelGGL(build_b_batch_kernel, dim3(nx, ny), dim3(256), 0, s, d_b_cat, d_prof_cat, dd, d_bad);
        }
        if (!hip_ok(hipGetLastError(), "profile kernels")) return false;
    }
    return true;
}

// How a rectangle of w words is cut into strips.  Chained strips all have the kernel's height (32*k words).  A sequential
// pair may finish with up to kMaxTail1[k] short strips of 32 words when that is cheaper than one mostly empty tall strip
// (a k = 1 step costs about 0.67 / 0.43 / 0.25 of a k = 2 / 4 / 8 step).
StripPlan strip_plan(int w, int k, bool sequential) {
    StripPlan p;
    const int wps = kWordsPerStrip * k;
    p.full = w / wps;
    const int r = w - p.full * wps;
    if (r == 0) return p;
    const int max_tail1 = !sequential ? 0 : (k == 2 ? 1 : (k == 4 ? 2 : (k >= 8 ? 3 : 0)));
    const int t1 = (r + kWordsPerStrip - 1) / kWordsPerStrip;
    if (t1 <= max_tail1) p.tail1 = t1;
    else p.full += 1;
    return p;
}

// Plan the strips of one rectangle: words [w0, w1) x n columns, r.k subwords per lane.
void plan_rect(std::vector<StripJob>& jobs, const RectPlan& r) {
    const int w = r.w1 - r.w0;
    const int wps = kWordsPerStrip * r.k;
    const StripPlan sp = strip_plan(w, r.k, r.pingpong);
    const int S = sp.strips();
    int word = 0;
    for (int s = 0; s < S; ++s) {
        StripJob j;
        std::memset(&j, 0, sizeof j);
        const bool tall = s < sp.full;
        j.k = tall ? r.k : 1;
        j.a_codes = r.a_codes;
        j.b_prof = r.b_prof;
        j.v = r.v;
        j.n = r.n;
        j.col0 = r.col0;
        j.word0 = r.w0 + word;
        const int words = std::min(tall ? wps : kWordsPerStrip, w - word);
        j.nlanes = 2 * words;
        j.flags = r.v_init_one ? kJobVInitOne : 0;
        j.tail_rows = -1;
        if (s == 0) {
            j.hin_arr = r.hin_arr;  // nullptr => +1
        } else {
            j.hin_gran = r.gran + (size_t)(r.pingpong ? ((s - 1) & 1) : (s - 1)) * r.gran_stride;
        }
        if (s + 1 < S) {
            j.hout_gran = r.gran + (size_t)(r.pingpong ? (s & 1) : s) * r.gran_stride;
            j.exact_tail = 1;  // full strips anyway
        } else {
            j.hout_arr = r.hout_arr;
            j.sum_out = r.sum_out;
            j.tail_rows = r.tail_rows;
            j.exact_tail = (r.exact_end || r.hout_arr) ? 1 : 0;
        }
        if (r.values) {
            j.values = r.values;
            j.fill_stride = r.fill_stride;
            j.fill_word0 = r.fill_word0 + word;
        }
        j.ckpt = r.ckpt;
        j.ckpt_stride = r.ckpt_stride;
        word += words;
        jobs.push_back(j);
    }
}

size_t rect_granules(int n, int w, int k, bool pingpong) {
    const int S = strip_plan(w, k, pingpong).strips();
    const size_t G = (size_t)(n + 31) / 32;  // one 8-byte granule per 32 columns per strip boundary
    const int rows = pingpong ? std::min(S - 1, 2) : S - 1;
    return S > 1 ? (size_t)rows * G : 0;
}

// Residency cap.  Every strip of a rectangle advances at the pace of the most crowded SIMD it touches, and the
// dispatcher does not balance SIMDs by itself.  Blocks are 4 wavefronts (one per SIMD of a CU); an unused dynamic-LDS
// request sized so that only `W = ceil(blocks / CUs)` blocks fit in a CU's 160 KB makes W the hard maximum of
// wavefronts per SIMD instead of an average.
static unsigned residency_lds_bytes(int blocks) {
    static const bool off = getenv("PA_STRIP_NO_LDS_CAP") != nullptr;
    if (off) return 0;
    const int cus = device_cus();
    const int W = (blocks + cus - 1) / cus;
    if (W > 7) return 0;  // beyond the register-file limit nothing is gained
    const unsigned lds_total = 160u * 1024u;
    return ((lds_total / (unsigned)(W + 1)) + 1024u) & ~1023u;  // W blocks fit, W + 1 do not
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set it once per (kernel, device), from any
// thread (the library is re-entrant; pa_set_device selects the device per thread).
static bool ensure_max_lds(const void* kern) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    if (!hip_ok(hipGetDevice(&dev), "hipGetDevice")) return false;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({kern, dev})) return true;
    if (!hip_ok(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), "hipFuncSetAttribute(max dynamic LDS)")) return false;
    done.insert({kern, dev});
    return true;
}

template <class Kern>
static bool launch_one(Kern kern, int grid, int block_waves, unsigned lds, hipStream_t s, const StripJob* d_jobs, int njobs,
                       uint32_t* d_ticket_err) {
    if (!ensure_max_lds(reinterpret_cast<const void*>(kern))) return false;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * block_waves), lds, s, d_jobs, njobs, d_ticket_err, d_ticket_err + 1);
    return hip_ok(hipGetLastError(), "strip_kernel launch");
}

bool launch_strips(const StripJob* d_jobs, int njobs, bool fill, uint32_t* d_ticket_err, hipStream_t s, bool zero_ticket, bool scatter,
                   int k, int block_waves, bool ckpt) {
    if (njobs == 0) return true;
    // d_ticket_err[0] = ticket, [1] = err
    if (zero_ticket && !hip_ok(hipMemsetAsync(d_ticket_err, 0, 2 * sizeof(uint32_t), s), "memset ticket")) return false;
    if (block_waves < 1 || block_waves > kStripMaxBlockWaves) block_waves = kStripBlockWaves;
    if (const char* e = getenv("PA_STRIP_BLOCK_WAVES")) block_waves = std::min(std::max(atoi(e), 1), kStripMaxBlockWaves);  // experiments
    if (k < 4 && block_waves > kStripBlockWaves) block_waves = kStripBlockWaves;  // (the k = 1, 2 kernels are built for 256 threads)
    const int grid = (njobs + block_waves - 1) / block_waves;  // one wave per job; jobs beyond residency queue behind their
                                                               // producers (ticket order)
    const unsigned lds = block_waves >= kStripBlockWaves ? residency_lds_bytes(grid) : 0;
    if ((scatter || fill) && (k != 1 || ckpt)) {
        set_error("fill / scatter strips are built for k = 1 without checkpoints only");
        return false;
    }
    // tall cost-only strips take their eq words from LDS: one slice per wavefront of the block
    static const bool no_ldseq = getenv("PA_STRIP_NO_LDSEQ") != nullptr;
    if (!no_ldseq && !scatter && !fill && (k == 4 || k == 8)) {
        const unsigned need = (unsigned)block_waves * (k == 8 ? LdsEq<8>::kWaveBytes : LdsEq<4>::kWaveBytes);
        const unsigned l = std::max(lds, need);
        if (ckpt && k == 4) return launch_one(strip_kernel<4, false, false, true, true>, grid, block_waves, l, s, d_jobs, njobs, d_ticket_err);
        if (ckpt && k == 8) return launch_one(strip_kernel<8, false, false, true, true>, grid, block_waves, l, s, d_jobs, njobs, d_ticket_err);
        if (k == 4) return launch_one(strip_kernel<4, false, false, false, true>, grid, block_waves, l, s, d_jobs, njobs, d_ticket_err);
        return launch_one(strip_kernel<8, false, false, false, true>, grid, block_waves, l, s, d_jobs, njobs, d_ticket_err);
    }
    if (ckpt) {
        if (k == 1) return launch_one(strip_kernel<1, false, false, true>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
        if (k == 2) return launch_one(strip_kernel<2, false, false, true>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
        if (k == 4) return launch_one(strip_kernel<4, false, false, true>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
        if (k == 8) return launch_one(strip_kernel<8, false, false, true>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
    }
    if (scatter && fill) return launch_one(strip_kernel<1, true, true>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
    if (scatter) return launch_one(strip_kernel<1, false, true>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
    if (fill) return launch_one(strip_kernel<1, true, false>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
    if (k == 1) return launch_one(strip_kernel<1, false, false>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
    if (k == 2) return launch_one(strip_kernel<2, false, false>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
    if (k == 4) return launch_one(strip_kernel<4, false, false>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
    if (k == 8) return launch_one(strip_kernel<8, false, false>, grid, block_waves, lds, s, d_jobs, njobs, d_ticket_err);
    set_error("unsupported strip height k=%d", k);
    return false;
}

template <int K, bool CKPT>
static bool launch_pairs_k(const StripJob* d_jobs, const int32_t* d_first, int npairs, uint32_t* d_err, hipStream_t s, int grid, unsigned lds) {
    // tall strips take their eq words from LDS (strip_kernel.hpp LdsEq): one slice per wavefront of the block
    static const bool no_ldseq = getenv("PA_PAIR_NO_LDSEQ") != nullptr;
    if (K >= 4 && !no_ldseq) {
        constexpr bool L = K >= 4;  // (keeps the K < 4 instantiations out of the binary)
        const unsigned need = (unsigned)kStripBlockWaves * LdsEq<K>::kWaveBytes;
        if (!ensure_max_lds(reinterpret_cast<const void*>(pair_kernel<K, CKPT, L>))) return false;
        hipLaunchKernelGGL((pair_kernel<K, CKPT, L>), dim3(grid), dim3(64 * kStripBlockWaves), std::max(lds, need), s, d_jobs, d_first, npairs, d_err);
        return hip_ok(hipGetLastError(), "pair_kernel launch");
    }
    if (!ensure_max_lds(reinterpret_cast<const void*>(pair_kernel<K, CKPT, false>))) return false;
    hipLaunchKernelGGL((pair_kernel<K, CKPT, false>), dim3(grid), dim3(64 * kStripBlockWaves), lds, s, d_jobs, d_first, npairs, d_err);
    return hip_ok(hipGetLastError(), "pair_kernel launch");
}

bool launch_pairs(const StripJob* d_jobs, const int32_t* d_first, int npairs, uint32_t* d_ticket_err, hipStream_t s, int k, bool ckpt) {
    if (npairs == 0) return true;
    const int grid = (npairs + kStripBlockWaves - 1) / kStripBlockWaves;
    const unsigned lds = residency_lds_bytes(grid);
    uint32_t* e = d_ticket_err + 1;
    if (!ckpt) {
        if (k == 1) return launch_pairs_k<1, false>(d_jobs, d_first, npairs, e, s, grid, lds);
        if (k == 2) return launch_pairs_k<2, false>(d_jobs, d_first, npairs, e, s, grid, lds);
        if (k == 4) return launch_pairs_k<4, false>(d_jobs, d_first, npairs, e, s, grid, lds);
        if (k == 8) return launch_pairs_k<8, false>(d_jobs, d_first, npairs, e, s, grid, lds);
        if (k == 16) return launch_pairs_k<16, false>(d_jobs, d_first, npairs, e, s, grid, 0);
    } else {
        if (k == 1) return launch_pairs_k<1, true>(d_jobs, d_first, npairs, e, s, grid, lds);
        if (k == 2) return launch_pairs_k<2, true>(d_jobs, d_first, npairs, e, s, grid, lds);
        if (k == 4) return launch_pairs_k<4, true>(d_jobs, d_first, npairs, e, s, grid, lds);
        if (k == 8) return launch_pairs_k<8, true>(d_jobs, d_first, npairs, e, s, grid, lds);
    }
    set_error("unsupported strip height k=%d", k);
    return false;
}

}  // namespace pa

using namespace pa;

extern "C" int pa_bp_profile_build(const uint8_t* a, size_t n, const uint8_t* b, size_t m, uint64_t* a2,
                                   uint64_t* b2) {
    if (!ensure_device()) return PA_E_HIP;
    const size_t w = (m + 63) / 64, cw = (n + 15) / 16;
    DeviceBuf d_a, d_b, d_codes, d_prof, d_bad;
    if (!d_a.alloc(n) || !d_b.alloc(m) || !d_codes.alloc(cw * 4) || !d_prof.alloc(w * 16) || !d_bad.alloc(4))
        return PA_E_HIP;
    hipStream_t s = 0;
    if (n && !hip_ok(hipMemcpyAsync(d_a.ptr, a, n, hipMemcpyHostToDevice, s), "H2D a")) return PA_E_HIP;
    if (m && !hip_ok(hipMemcpyAsync(d_b.ptr, b, m, hipMemcpyHostToDevice, s), "H2D b")) return PA_E_HIP;
    if (!hip_ok(hipMemsetAsync(d_bad.ptr, 0, 4, s), "memset")) return PA_E_HIP;
    if (!encode_a_device(d_a.as<uint8_t>(), (int)n, d_codes.as<uint32_t>(), d_bad.as<uint32_t>(), s)) return PA_E_HIP;
    if (!build_b_device(d_b.as<uint8_t>(), (int)m, d_prof.as<uint64_t>(), d_bad.as<uint32_t>(), s)) return PA_E_HIP;
    std::vector<uint32_t> codes(cw);
    uint32_t bad = 0;
    if (cw && !hip_ok(hipMemcpyAsync(codes.data(), d_codes.ptr, cw * 4, hipMemcpyDeviceToHost, s), "D2H codes")) return PA_E_HIP;
    if (w && !hip_ok(hipMemcpyAsync(b2, d_prof.ptr, w * 16, hipMemcpyDeviceToHost, s), "D2H prof")) return PA_E_HIP;
    if (!hip_ok(hipMemcpyAsync(&bad, d_bad.ptr, 4, hipMemcpyDeviceToHost, s), "D2H bad")) return PA_E_HIP;
    if (!hip_ok(hipStreamSynchronize(s), "sync")) return PA_E_HIP;
    if (bad) {
        set_error("sequence contains a base outside ACGT");
        return PA_E_INVALID_BASE;
    }
    for (size_t i = 0; i < n; ++i) {  // exploded Bits of a (profile.rs:116-125)
        const uint32_t r = (codes[i / 16] >> (2 * (i % 16))) & 3u;
        a2[2 * i] = 0ull - (uint64_t)(r & 1);
        a2[2 * i + 1] = 0ull - (uint64_t)((r >> 1) & 1);
    }
    return 0;
}

// Shared implementation of pa_bp_compute / pa_bp_fill on host buffers.
static int32_t rect_host(const uint64_t* a2, size_t n, const uint64_t* b2, size_t w, uint64_t* h2, uint64_t* v2,
                         int exact_end, uint64_t* values) {
    if (!ensure_device()) return INT32_MIN;
    if (n > (size_t)INT32_MAX / 2 || w > (size_t)INT32_MAX / 64) {
        set_error("rectangle too large");
        return INT32_MIN;
    }
    if (n == 0) return 0;
    if (w == 0) {  // no rows: bottom == top
        int32_t s = 0;
        for (size_t i = 0; i < n; ++i) s += (int32_t)h2[2 * i] - (int32_t)h2[2 * i + 1];
        return s;
    }
    const size_t cw = (n + 15) / 16;
    std::vector<uint32_t> codes(cw, 0);
    std::vector<uint8_t> hin(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t r = (uint32_t)(a2[2 * i] & 1) | ((uint32_t)(a2[2 * i + 1] & 1) << 1);
        codes[i / 16] |= r << (2 * (i % 16));
        hin[i] = (uint8_t)((h2[2 * i] & 1) | ((h2[2 * i + 1] & 1) << 1));
    }
    const size_t ngran = rect_granules((int)n, (int)w);
    DeviceBuf d_codes, d_prof, d_v, d_hin, d_hout, d_gran, d_jobs, d_misc, d_values;
    if (!d_codes.alloc(cw * 4) || !d_prof.alloc(w * 16) || !d_v.alloc(w * 16) || !d_hin.alloc(n) ||
        !d_hout.alloc(n) || !d_gran.alloc(ngran * 8) || !d_misc.alloc(16))
        return INT32_MIN;
    if (values && !d_values.alloc(n * w * 16)) return INT32_MIN;
    hipStream_t s = 0;
    bool ok = hip_ok(hipMemcpyAsync(d_codes.ptr, codes.data(), cw * 4, hipMemcpyHostToDevice, s), "H2D") &&
              hip_ok(hipMemcpyAsync(d_prof.ptr, b2, w * 16, hipMemcpyHostToDevice, s), "H2D") &&
              hip_ok(hipMemcpyAsync(d_v.ptr, v2, w * 16, hipMemcpyHostToDevice, s), "H2D") &&
              hip_ok(hipMemcpyAsync(d_hin.ptr, hin.data(), n, hipMemcpyHostToDevice, s), "H2D") &&
              hip_ok(hipMemsetAsync(d_gran.ptr, 0, std::max<size_t>(ngran * 8, 16), s), "memset gran") &&
              hip_ok(hipMemsetAsync(d_misc.ptr, 0, 16, s), "memset misc");
    if (!ok) return INT32_MIN;

    std::vector<StripJob> jobs;
    RectPlan r;
    r.a_codes = d_codes.as<uint32_t>();
    r.b_prof = d_prof.as<uint32_t>();
    r.v = d_v.as<uint32_t>();
    r.n = (int)n;
    r.w0 = 0;
    r.w1 = (int)w;
    r.hin_arr = d_hin.as<uint8_t>();
    r.hout_arr = d_hout.as<uint8_t>();
    r.gran = d_gran.as<uint64_t>();
    r.gran_stride = (n + 31) / 32;
    r.sum_out = d_misc.as<int32_t>() + 2;
    r.exact_end = exact_end != 0 || values != nullptr;
    if (!exact_end && !values) r.hout_arr = nullptr;  // padded-tail path: the bottom row itself is not an output
    r.values = values ? d_values.as<uint32_t>() : nullptr;
    r.fill_stride = (int)w;
    r.fill_word0 = 0;
    plan_rect(jobs, r);
    if (!d_jobs.alloc(jobs.size() * sizeof(StripJob))) return INT32_MIN;
    ok = hip_ok(hipMemcpyAsync(d_jobs.ptr, jobs.data(), jobs.size() * sizeof(StripJob), hipMemcpyHostToDevice, s), "H2D jobs") &&
         launch_strips(d_jobs.as<StripJob>(), (int)jobs.size(), values != nullptr, d_misc.as<uint32_t>(), s);
    if (!ok) return INT32_MIN;
    uint32_t misc[4] = {0, 0, 0, 0};
    std::vector<uint8_t> hout(n, 0);
    ok = hip_ok(hipMemcpyAsync(misc, d_misc.ptr, 16, hipMemcpyDeviceToHost, s), "D2H") &&
         hip_ok(hipMemcpyAsync(v2, d_v.ptr, w * 16, hipMemcpyDeviceToHost, s), "D2H") &&
         (r.hout_arr == nullptr || hip_ok(hipMemcpyAsync(hout.data(), d_hout.ptr, n, hipMemcpyDeviceToHost, s), "D2H")) &&
         (!values || hip_ok(hipMemcpyAsync(values, d_values.ptr, n * w * 16, hipMemcpyDeviceToHost, s), "D2H values")) &&
         hip_ok(hipStreamSynchronize(s), "sync");
    if (!ok) return INT32_MIN;
    if (misc[1] != PA_ERR_NONE) {
        set_error("device spin timeout (err=%u)", misc[1]);
        return INT32_MIN;
    }
    if (r.hout_arr) {
        for (size_t i = 0; i < n; ++i) {
            const uint32_t x = hout[i] & 3u;
            h2[2 * i] = x & 1;
            h2[2 * i + 1] = x >> 1;
        }
    }
    // exact_end == 0: the reference leaves h unspecified (simd.rs:184-225); h2 is left untouched.
    return (int32_t)misc[2];
}

extern "C" int32_t pa_bp_compute(const uint64_t* a2, size_t n, const uint64_t* b2, size_t w, uint64_t* h2, uint64_t* v2,
                                 int exact_end) {
    return rect_host(a2, n, b2, w, h2, v2, exact_end, nullptr);
}

extern "C" int32_t pa_bp_fill(const uint64_t* a2, size_t n, const uint64_t* b2, size_t w, uint64_t* h2, uint64_t* v2,
                              uint64_t* values) {
    return rect_host(a2, n, b2, w, h2, v2, 1, values);
}
