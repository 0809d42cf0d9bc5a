// search_batch_unit.hip -- batched semi-global search (pa_search_batch_*, include/pa_bitpacking_hip.h).
//
// Patterns and texts are uploaded once; a query names one of each.  One run() launches
//   * seg_kernel for every query whose pattern fits one strip (plen <= 2048): several queries per wavefront, sorted by
//     (segment width g, text length) so that the queries of a wave end at about the same column;
//   * the chained scatter-profile strips of pa_search (plan_rect, strip_kernel<1, false, true>) for longer patterns;
//   * search_best_kernel: best hit of every query.
// trace() re-fills text[end - min(end, 2 plen) .. end) x pattern of every query with the FILL strips in one launch per chunk of
// queries (the `values` columns are bounded by a device-memory budget) and walks the paths on the GPU.
#include "pa_hip_internal.hpp"
#include "engine.hpp"
#include "search_batch_kernel.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

using namespace pa;
using namespace pa::search_batch;

namespace {

constexpr size_t kMaxLen = size_t(1) << 30;
constexpr size_t kSegMaxRows = 64 * 32;  // one strip: 64 lanes of 32 rows

int seg_lg(size_t plen) {  // log2 of the segment width: smallest g = 2^lg with 32 g >= max(plen, 1)
    int lg = 0;
    while ((size_t(32) << lg) < plen) ++lg;
    return lg;
}

bool text_ok(const uint8_t* t, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const uint8_t ch = t[i] & 0xDF;
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') return false;
    }
    return true;
}

int32_t v_value(uint64_t p, uint64_t m) { return (int32_t)__builtin_popcountll(p) - (int32_t)__builtin_popcountll(m); }

int32_t value_to_host(const uint64_t* v, int64_t j) {  // V::value_to
    int32_t s = 0;
    for (int64_t k = 0; k < j / 64; ++k) s += v_value(v[2 * k], v[2 * k + 1]);
    if (j % 64 != 0) {
        const uint64_t mask = (1ull << (j % 64)) - 1;
        s += v_value(v[2 * (j / 64)] & mask, v[2 * (j / 64) + 1] & mask);
    }
    return s;
}

int32_t vrow_host(const uint64_t* v, size_t r) {
    return (int32_t)((v[2 * (r / 64)] >> (r % 64)) & 1) - (int32_t)((v[2 * (r / 64) + 1] >> (r % 64)) & 1);
}

}  // namespace

struct pa_search_batch {
    size_t npat = 0, ntext = 0, nq = 0;
    float uc = 0;
    std::vector<size_t> plen, tlen;
    std::vector<uint32_t> qp, qt;
    // host copies: the pattern profiles and left columns (traceback), per-pattern word offsets and widths
    std::vector<uint64_t> prof, v0;  // 4 resp. 2 u64 per word
    std::vector<size_t> prof_word, pat_words;
    std::vector<size_t> code_word;  // per text: first u32 of its codes
    DeviceBuf d_codes, d_prof, d_v0, d_zero;
    // forward plan
    bool no_pack = false;
    std::vector<int> lg;  // per query: segment width log2, -1 = chained strips
    std::vector<SegWave> waves;
    std::vector<SegQuery> segq;
    std::vector<RedQuery> redq;  // in query order
    std::vector<StripJob> jobs;
    std::vector<uint32_t> chained;  // queries on chained strips
    std::vector<size_t> v_word;     // per query: first V word of its output column in d_v
    size_t gran_words = 0, bot_bytes = 0, v_words = 0;
    DeviceBuf d_waves, d_segq, d_redq, d_jobs, d_bot, d_v, d_gran, d_misc, d_best_cost, d_best_idx, d_copy;
    std::vector<uint64_t> copy_desc;  // chained queries: (v0 word, v word, words) triples
    double lanes_real = 0;
    bool ran = false;
    std::vector<int32_t> best_cost;
    std::vector<uint64_t> best_idx;
};

namespace {

// chained strips start from v0: copy it into their output columns (one wave per query)
__global__ void copy_v0_kernel(const uint64_t* __restrict__ desc, int n, const uint64_t* __restrict__ v0, uint64_t* __restrict__ v) {
    const int q = (int)blockIdx.x;
    if (q >= n) return;
    const uint64_t src = desc[3 * q], dst = desc[3 * q + 1], words = desc[3 * q + 2];
    for (uint64_t i = threadIdx.x; i < 2 * words; i += blockDim.x) v[2 * dst + i] = v0[2 * src + i];
}

int check_device_error(const DeviceBuf& d_misc, hipStream_t s) {
    uint32_t misc[2] = {0, 0};
    if (!hip_ok(hipMemcpyAsync(misc, d_misc.ptr, 8, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    if (misc[1] != PA_ERR_NONE) return fail(PA_E_TIMEOUT, "device spin timeout (err=%u)", misc[1]);
    return 0;
}

int build(pa_search_batch& sb, const uint8_t* const* patterns, const uint8_t* const* texts) {
    hipStream_t s = 0;
    // texts: host-encoded codes (A0 C1 T2 G3, the order of the ScatterProfile), each text on whole u32 words
    std::vector<uint32_t> codes;
    sb.code_word.resize(sb.ntext);
    size_t max_t = 0;
    for (size_t t = 0; t < sb.ntext; ++t) {
        sb.code_word[t] = codes.size();
        const size_t n = sb.tlen[t];
        max_t = std::max(max_t, n);
        codes.resize(codes.size() + (n + 15) / 16 + 1, 0);
        uint32_t* w = codes.data() + sb.code_word[t];
        for (size_t i = 0; i < n; ++i) {
            const uint8_t ch = texts[t][i] & 0xDF;
            const uint32_t c = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'T' ? 2 : 3;
            w[i / 16] |= c << (2 * (i % 16));
        }
    }
    // patterns: profile and left column, at least one strip segment's worth of words (padding rows match everything, v0 = 0 there)
    sb.prof_word.resize(sb.npat);
    sb.pat_words.resize(sb.npat);
    std::vector<uint64_t> pr, v0;
    std::vector<bool> used(sb.npat, false);
    for (uint32_t p : sb.qp) used[p] = true;
    for (size_t p = 0; p < sb.npat; ++p) {
        const size_t w = (sb.plen[p] + 63) / 64;
        size_t words = std::max<size_t>(w, 1);
        if (sb.plen[p] <= kSegMaxRows) words = std::max<size_t>(words, ((size_t(32) << seg_lg(sb.plen[p])) + 63) / 64);
        if (!used[p]) {  // (not validated: no query reads it)
            sb.prof_word[p] = sb.prof.size() / 4;
            sb.pat_words[p] = 0;
            continue;
        }
        if (const int rc = search_profile(patterns[p], sb.plen[p], sb.uc, pr, v0)) return rc;
        if (sb.plen[p] == 0) std::fill(pr.begin(), pr.end(), ~0ull);  // no pattern row: every row is padding
        pr.resize(4 * words, ~0ull);
        v0.resize(2 * words, 0);
        sb.prof_word[p] = sb.prof.size() / 4;
        sb.pat_words[p] = words;
        sb.prof.insert(sb.prof.end(), pr.begin(), pr.end());
        sb.v0.insert(sb.v0.end(), v0.begin(), v0.end());
    }
    if (!upload(sb.d_codes, codes.data(), codes.size() * 4, s) || !upload(sb.d_prof, sb.prof.data(), sb.prof.size() * 8, s) ||
        !upload(sb.d_v0, sb.v0.data(), sb.v0.size() * 8, s) || !sb.d_zero.alloc(max_t + 64) ||
        !hip_ok(hipMemsetAsync(sb.d_zero.ptr, 0, max_t + 64, s), "memset"))
        return PA_E_HIP;

    // ---- forward plan ----
    sb.lg.assign(sb.nq, -1);
    std::vector<uint32_t> packed;
    for (size_t q = 0; q < sb.nq; ++q) {
        const size_t pl = sb.plen[sb.qp[q]];
        sb.lanes_real += (double)((pl + 31) / 32);
        if (!sb.no_pack && pl <= kSegMaxRows) {
            sb.lg[q] = seg_lg(pl);
            packed.push_back((uint32_t)q);
        } else {
            sb.chained.push_back((uint32_t)q);
        }
    }
    std::stable_sort(packed.begin(), packed.end(), [&](uint32_t a, uint32_t b) {
        return sb.lg[a] != sb.lg[b] ? sb.lg[a] < sb.lg[b] : sb.tlen[sb.qt[a]] < sb.tlen[sb.qt[b]];
    });
    // output areas: bottom rows (u64 chunks of the segment kernel, one byte per column of the strips) and final columns
    std::vector<size_t> bot_off(sb.nq, 0);
    sb.v_word.assign(sb.nq, 0);
    for (size_t q = 0; q < sb.nq; ++q) {
        const size_t n = sb.tlen[sb.qt[q]];
        bot_off[q] = sb.bot_bytes;
        sb.v_word[q] = sb.v_words;
        if (sb.lg[q] >= 0) {
            sb.bot_bytes += 8 * ((n + (size_t(1) << sb.lg[q]) + 31) / 32);
            sb.v_words += sb.pat_words[sb.qp[q]];
        } else {
            sb.bot_bytes += (n + 7) & ~size_t(7);
            sb.v_words += std::max<size_t>((sb.plen[sb.qp[q]] + 63) / 64, 1);
        }
    }
    if (!sb.d_bot.alloc(std::max<size_t>(sb.bot_bytes, 16)) || !sb.d_v.alloc(std::max<size_t>(sb.v_words * 16, 16)) ||
        !hip_ok(hipMemsetAsync(sb.d_bot.ptr, 0, std::max<size_t>(sb.bot_bytes, 16), s), "memset") ||
        !hip_ok(hipMemsetAsync(sb.d_v.ptr, 0, std::max<size_t>(sb.v_words * 16, 16), s), "memset"))
        return PA_E_HIP;
    const uint32_t* codes_d = sb.d_codes.as<uint32_t>();
    const uint64_t* prof_d = sb.d_prof.as<uint64_t>();
    const uint64_t* v0_d = sb.d_v0.as<uint64_t>();
    uint64_t* v_d = sb.d_v.as<uint64_t>();
    uint8_t* bot_d = sb.d_bot.as<uint8_t>();
    // segment waves: 64 / g queries of one width, in (g, tlen) order
    for (size_t i = 0; i < packed.size();) {
        const int l = sb.lg[packed[i]];
        const size_t per = size_t(64) >> l;
        SegWave W;
        W.first = (uint32_t)sb.segq.size();
        W.lg = (uint32_t)l;
        W.nq = 0;
        W.tmin = UINT32_MAX;
        W.tmax = 0;
        while (i < packed.size() && sb.lg[packed[i]] == l && W.nq < per) {
            const uint32_t q = packed[i++];
            const size_t p = sb.qp[q], n = sb.tlen[sb.qt[q]];
            SegQuery Q;
            std::memset(&Q, 0, sizeof Q);
            Q.codes = codes_d + sb.code_word[sb.qt[q]];
            Q.prof = reinterpret_cast<const uint32_t*>(prof_d + 4 * sb.prof_word[p]);
            Q.v0 = reinterpret_cast<const uint32_t*>(v0_d + 2 * sb.prof_word[p]);
            Q.v = reinterpret_cast<uint32_t*>(v_d + 2 * sb.v_word[q]);
            Q.bot = reinterpret_cast<uint64_t*>(bot_d + bot_off[q]);
            Q.tlen = (uint32_t)n;
            sb.segq.push_back(Q);
            W.tmin = std::min<uint32_t>(W.tmin, (uint32_t)n);
            W.tmax = std::max<uint32_t>(W.tmax, (uint32_t)n);
            ++W.nq;
        }
        sb.waves.push_back(W);
    }
    // chained strips, one rectangle per query (the plan of pa_search)
    std::vector<size_t> gran_off;
    for (uint32_t q : sb.chained) {
        const size_t n = sb.tlen[sb.qt[q]], w = (sb.plen[sb.qp[q]] + 63) / 64;
        gran_off.push_back(sb.gran_words);
        if (n > 0 && w > 0) sb.gran_words += rect_granules((int)n, (int)w);
        sb.copy_desc.insert(sb.copy_desc.end(), {(uint64_t)sb.prof_word[sb.qp[q]], (uint64_t)sb.v_word[q], (uint64_t)std::max<size_t>(w, 1)});
    }
    if (!sb.d_gran.alloc(std::max<size_t>(sb.gran_words * 8, 16)) || !sb.d_misc.alloc(16)) return PA_E_HIP;
    for (size_t k = 0; k < sb.chained.size(); ++k) {
        const uint32_t q = sb.chained[k];
        const size_t p = sb.qp[q], n = sb.tlen[sb.qt[q]], w = (sb.plen[p] + 63) / 64;
        if (n == 0 || w == 0) continue;  // nothing to compute: the bottom row is the top row (0), the column stays v0
        RectPlan r;
        r.a_codes = codes_d + sb.code_word[sb.qt[q]];
        r.b_prof = reinterpret_cast<const uint32_t*>(prof_d + 4 * sb.prof_word[p]);
        r.v = reinterpret_cast<uint32_t*>(v_d + 2 * sb.v_word[q]);
        r.n = (int)n;
        r.w0 = 0;
        r.w1 = (int)w;
        r.hin_arr = sb.d_zero.as<uint8_t>();  // zeros along the top: the match may start anywhere
        r.hout_arr = bot_d + bot_off[q];
        r.gran = sb.d_gran.as<uint64_t>() + gran_off[k];
        r.gran_stride = (n + 31) / 32;
        r.exact_end = true;
        plan_rect(sb.jobs, r);
    }
    // best-hit reduction, in query order
    sb.redq.resize(sb.nq);
    for (size_t q = 0; q < sb.nq; ++q) {
        const size_t p = sb.qp[q];
        RedQuery R;
        std::memset(&R, 0, sizeof R);
        R.tlen = (uint32_t)sb.tlen[sb.qt[q]];
        R.plen = (uint32_t)sb.plen[p];
        R.v = reinterpret_cast<const uint32_t*>(v_d + 2 * sb.v_word[q]);
        R.v0 = reinterpret_cast<const uint32_t*>(v0_d + 2 * sb.prof_word[p]);
        if (sb.lg[q] >= 0) {
            R.g = 1u << sb.lg[q];
            R.rows = 32u * R.g;
            R.bot = reinterpret_cast<const uint64_t*>(bot_d + bot_off[q]);
        } else {
            R.g = 0;
            R.rows = (uint32_t)(64 * ((sb.plen[p] + 63) / 64));
            R.bytes = bot_d + bot_off[q];
        }
        sb.redq[q] = R;
    }
    if (!upload(sb.d_waves, sb.waves.data(), sb.waves.size() * sizeof(SegWave), s) ||
        !upload(sb.d_segq, sb.segq.data(), sb.segq.size() * sizeof(SegQuery), s) ||
        !upload(sb.d_redq, sb.redq.data(), sb.redq.size() * sizeof(RedQuery), s) ||
        !upload(sb.d_jobs, sb.jobs.data(), sb.jobs.size() * sizeof(StripJob), s) ||
        !upload(sb.d_copy, sb.copy_desc.data(), sb.copy_desc.size() * 8, s) || !sb.d_best_cost.alloc(std::max<size_t>(sb.nq, 1) * 4) ||
        !sb.d_best_idx.alloc(std::max<size_t>(sb.nq, 1) * 8) || !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    return 0;
}

bool launch_best(const pa_search_batch& sb, const uint64_t* d_want, int32_t* d_want_val, hipStream_t s) {
    if (sb.nq == 0) return true;
    const int grid = (int)((sb.nq + kSegBlockWaves - 1) / kSegBlockWaves);
    hipLaunchKernelGGL(search_best_kernel, dim3(grid), dim3(64 * kSegBlockWaves), 0, s, sb.d_redq.as<RedQuery>(), (int)sb.nq,
                       sb.d_best_cost.as<int32_t>(), sb.d_best_idx.as<uint64_t>(), d_want, d_want_val);
    return hip_ok(hipGetLastError(), "search_best_kernel launch");
}

int forward(pa_search_batch& sb, float* kernel_ms) {
    hipStream_t s = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!hip_ok(hipEventCreate(&e0), "hipEventCreate") || !hip_ok(hipEventCreate(&e1), "hipEventCreate")) return PA_E_HIP;
    struct EventGuard {
        hipEvent_t a, b;
        ~EventGuard() {
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
        }
    } guard{e0, e1};
    bool ok = hip_ok(hipMemsetAsync(sb.d_gran.ptr, 0, std::max<size_t>(sb.gran_words * 8, 16), s), "memset gran") &&
              hip_ok(hipMemsetAsync(sb.d_misc.ptr, 0, 16, s), "memset misc");
    if (ok && !sb.chained.empty()) {
        hipLaunchKernelGGL(copy_v0_kernel, dim3((unsigned)sb.chained.size()), dim3(64), 0, s, sb.d_copy.as<uint64_t>(), (int)sb.chained.size(),
                           sb.d_v0.as<uint64_t>(), sb.d_v.as<uint64_t>());
        ok = hip_ok(hipGetLastError(), "copy_v0_kernel launch");
    }
    ok = ok && hip_ok(hipEventRecord(e0, s), "event");
    if (ok && !sb.waves.empty()) {
        const int grid = (int)((sb.waves.size() + kSegBlockWaves - 1) / kSegBlockWaves);
        hipLaunchKernelGGL(seg_kernel, dim3(grid), dim3(64 * kSegBlockWaves), 0, s, sb.d_waves.as<SegWave>(), (int)sb.waves.size(),
                           sb.d_segq.as<SegQuery>());
        ok = hip_ok(hipGetLastError(), "seg_kernel launch");
    }
    ok = ok && launch_strips(sb.d_jobs.as<StripJob>(), (int)sb.jobs.size(), false, sb.d_misc.as<uint32_t>(), s, true, /*scatter=*/true) &&
         launch_best(sb, nullptr, nullptr, s) && hip_ok(hipEventRecord(e1, s), "event");
    if (!ok) return PA_E_HIP;
    sb.best_cost.assign(sb.nq, 0);
    sb.best_idx.assign(sb.nq, 0);
    ok = (sb.nq == 0 || (hip_ok(hipMemcpyAsync(sb.best_cost.data(), sb.d_best_cost.ptr, sb.nq * 4, hipMemcpyDeviceToHost, s), "D2H") &&
                         hip_ok(hipMemcpyAsync(sb.best_idx.data(), sb.d_best_idx.ptr, sb.nq * 8, hipMemcpyDeviceToHost, s), "D2H"))) &&
         hip_ok(hipStreamSynchronize(s), "sync");
    if (!ok) return PA_E_HIP;
    if (const int rc = check_device_error(sb.d_misc, s)) return rc;
    if (kernel_ms) {
        float ms = 0;
        if (!hip_ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime")) return PA_E_HIP;
        *kernel_ms = ms;
    }
    sb.ran = true;
    return 0;
}

struct TraceItem {
    uint32_t q;
    size_t pi, pj, start, end, w;
    int32_t target;
    size_t values_bytes, gran_words, ops;
};

}  // namespace

extern "C" pa_search_batch* pa_search_batch_create(const uint8_t* const* patterns, const size_t* plens, size_t npatterns,
                                                   const uint8_t* const* texts, const size_t* tlens, size_t ntexts, const uint32_t* q_pattern,
                                                   const uint32_t* q_text, size_t nqueries, float unmatched_cost) {
    if (!(unmatched_cost >= 0.0f && unmatched_cost <= 1.0f)) {
        set_error("pa_search_batch_create: unmatched_cost must be in [0, 1]");
        return nullptr;
    }
    if ((npatterns && (!patterns || !plens)) || (ntexts && (!texts || !tlens)) || (nqueries && (!q_pattern || !q_text))) {
        set_error("pa_search_batch_create: NULL array");
        return nullptr;
    }
    for (size_t p = 0; p < npatterns; ++p)
        if (plens[p] > kMaxLen || (plens[p] && !patterns[p])) {
            set_error("pa_search_batch_create: pattern %zu: length above 2^30 or NULL", p);
            return nullptr;
        }
    for (size_t t = 0; t < ntexts; ++t)
        if (tlens[t] > kMaxLen || (tlens[t] && !texts[t])) {
            set_error("pa_search_batch_create: text %zu: length above 2^30 or NULL", t);
            return nullptr;
        }
    for (size_t q = 0; q < nqueries; ++q)
        if (q_pattern[q] >= npatterns || q_text[q] >= ntexts) {
            set_error("pa_search_batch_create: query %zu: pattern %u / text %u out of range", q, q_pattern[q], q_text[q]);
            return nullptr;
        }
    // bad characters, reported for the first query that uses them
    std::vector<int8_t> pat_ok(npatterns, -1), txt_ok(ntexts, -1);
    std::vector<uint64_t> pr, v0;
    for (size_t q = 0; q < nqueries; ++q) {
        const uint32_t p = q_pattern[q], t = q_text[q];
        if (pat_ok[p] < 0) {
            pat_ok[p] = 1;
            for (size_t j = 0; j < plens[p] && pat_ok[p]; ++j)
                if (!std::strchr("ACGTNYR*acgtnyr", patterns[p][j]) || patterns[p][j] == 0) pat_ok[p] = 0;
        }
        if (txt_ok[t] < 0) txt_ok[t] = text_ok(texts[t], tlens[t]) ? 1 : 0;
        if (!pat_ok[p]) {
            set_error("pa_search_batch_create: query %zu: unknown base in pattern %u", q, p);
            return nullptr;
        }
        if (!txt_ok[t]) {
            set_error("pa_search_batch_create: query %zu: text %u must be actgACTG only", q, t);
            return nullptr;
        }
    }
    if (!ensure_device()) return nullptr;
    pa_search_batch* sb = new (std::nothrow) pa_search_batch;
    if (!sb) {
        set_error("out of memory");
        return nullptr;
    }
    sb->npat = npatterns;
    sb->ntext = ntexts;
    sb->nq = nqueries;
    sb->uc = unmatched_cost;
    sb->plen.assign(plens, plens + npatterns);
    sb->tlen.assign(tlens, tlens + ntexts);
    sb->qp.assign(q_pattern, q_pattern + nqueries);
    sb->qt.assign(q_text, q_text + nqueries);
    const char* np = getenv("PA_SEARCH_BATCH_NO_PACK");
    sb->no_pack = np && *np && std::strcmp(np, "0") != 0;
    if (build(*sb, patterns, texts) != 0) {
        delete sb;
        return nullptr;
    }
    return sb;
}

extern "C" int pa_search_batch_run(pa_search_batch* sb, int32_t* best_cost, uint64_t* best_idx, float* kernel_ms) {
    if (!sb) return fail(PA_E_ARG, "pa_search_batch_run: NULL batch");
    if (kernel_ms) *kernel_ms = 0;
    if (const int rc = forward(*sb, kernel_ms)) return rc;
    if (best_cost && sb->nq) std::memcpy(best_cost, sb->best_cost.data(), sb->nq * 4);
    if (best_idx && sb->nq) std::memcpy(best_idx, sb->best_idx.data(), sb->nq * 8);
    return 0;
}

// out + offsets[q] receives query q's plen + tlen + 1 values (offsets[q] == UINT64_MAX: skip query q).  Assembled on the host from the
// device's bottom rows and final columns with the arithmetic of search_out (search_unit.hip).
extern "C" int pa_search_batch_rows(const pa_search_batch* sb, int32_t* out, const uint64_t* offsets) {
    if (!sb) return fail(PA_E_ARG, "pa_search_batch_rows: NULL batch");
    if (!sb->ran) return fail(PA_E_ARG, "pa_search_batch_rows: call pa_search_batch_run first");
    if (sb->nq == 0) return 0;
    if (!out || !offsets) return fail(PA_E_ARG, "pa_search_batch_rows: NULL output");
    std::vector<uint8_t> bot(sb->bot_bytes);
    std::vector<uint64_t> v(2 * sb->v_words);
    hipStream_t s = 0;
    if ((sb->bot_bytes && !hip_ok(hipMemcpyAsync(bot.data(), sb->d_bot.ptr, sb->bot_bytes, hipMemcpyDeviceToHost, s), "D2H")) ||
        (sb->v_words && !hip_ok(hipMemcpyAsync(v.data(), sb->d_v.ptr, sb->v_words * 16, hipMemcpyDeviceToHost, s), "D2H")) ||
        !hip_ok(hipStreamSynchronize(s), "sync"))
        return PA_E_HIP;
    const uint8_t* bot_base = sb->d_bot.as<uint8_t>();
    for (size_t q = 0; q < sb->nq; ++q) {
        if (offsets[q] == UINT64_MAX) continue;
        const RedQuery& R = sb->redq[q];
        const size_t n = R.tlen, rows = R.rows, pad = rows - R.plen;
        const uint64_t* vq = v.data() + 2 * sb->v_word[q];
        const uint64_t* v0q = sb->v0.data() + 2 * sb->prof_word[sb->qp[q]];
        const uint8_t* bq = bot.data() + ((R.g ? (const uint8_t*)R.bot : R.bytes) - bot_base);
        int32_t* o = out + offsets[q];
        size_t k = 0, skipped = 0;
        int32_t bsum = 0;
        for (size_t r = 0; r < rows; ++r) bsum += vrow_host(v0q, r);
        o[k++] = bsum;
        for (size_t c = 0; c < n; ++c) {
            if (R.g) {
                const size_t e = c + R.g, kk = e & 31;
                uint64_t x;
                std::memcpy(&x, bq + 8 * (e >> 5), 8);
                const unsigned pb = kk < 16 ? 31 - 2 * (unsigned)kk : 95 - 2 * (unsigned)kk;
                bsum += (int32_t)((x >> pb) & 1) - (int32_t)((x >> (pb - 1)) & 1);
            } else {
                bsum += (int32_t)(bq[c] & 1) - (int32_t)((bq[c] >> 1) & 1);
            }
            if (skipped < pad) skipped++;
            else o[k++] = bsum;
        }
        for (size_t j = 1; j <= rows; ++j) {
            bsum -= vrow_host(vq, rows - j) - vrow_host(v0q, rows - j);
            if (skipped < pad) skipped++;
            else o[k++] = bsum;
        }
        if (k != R.plen + n + 1) return fail(PA_E_INTERNAL, "pa_search_batch_rows: query %zu: internal length mismatch", q);
    }
    return 0;
}

extern "C" int pa_search_batch_trace(pa_search_batch* sb, const uint64_t* idx, char** cigars_out, int64_t* start_out) {
    if (!sb) return fail(PA_E_ARG, "pa_search_batch_trace: NULL batch");
    const size_t nq = sb->nq;
    if (cigars_out)
        for (size_t q = 0; q < nq; ++q) cigars_out[q] = nullptr;
    if (idx)
        for (size_t q = 0; q < nq; ++q)
            if (idx[q] > sb->plen[sb->qp[q]] + sb->tlen[sb->qt[q]])
                return fail(PA_E_ARG, "pa_search_batch_trace: query %zu: idx %llu out of range", q, (unsigned long long)idx[q]);
    if (nq == 0) return 0;
    if (!sb->ran)
        if (const int rc = forward(*sb, nullptr)) return rc;
    hipStream_t s = 0;
    // out[idx] of every query: the best hits' costs, or one more pass of the reduction
    std::vector<uint64_t> want(nq);
    std::vector<int32_t> val(nq);
    if (idx) {
        want.assign(idx, idx + nq);
        DeviceBuf d_want, d_val;
        if (!upload(d_want, want.data(), nq * 8, s) || !d_val.alloc(nq * 4) || !launch_best(*sb, d_want.as<uint64_t>(), d_val.as<int32_t>(), s) ||
            !hip_ok(hipMemcpyAsync(val.data(), d_val.ptr, nq * 4, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
    } else {
        want = sb->best_idx;
        val = sb->best_cost;
    }
    // per query: the window text[start .. end) x pattern, its target cost D[pj][pi] and its device footprint
    std::vector<TraceItem> items(nq);
    for (size_t q = 0; q < nq; ++q) {
        TraceItem& it = items[q];
        const size_t plen = sb->plen[sb->qp[q]], tlen = sb->tlen[sb->qt[q]], id = want[q];
        it.q = (uint32_t)q;
        if (id <= tlen) {
            it.pi = id;
            it.pj = plen;
        } else {
            it.pi = tlen;
            it.pj = plen - (id - tlen);
        }
        it.w = (plen + 63) / 64;
        const uint64_t* v0q = sb->v0.data() + 2 * sb->prof_word[sb->qp[q]];
        // out[idx] = D[pj][pi] + (unmatched cost of the rows below pj when the hit is in the right column)
        it.target = val[q] - (it.pi == tlen ? value_to_host(v0q, (int64_t)(64 * it.w)) - value_to_host(v0q, (int64_t)it.pj) : 0);
        it.end = it.pi;
        it.start = it.end > 2 * plen ? it.end - 2 * plen : 0;
        const size_t n = it.end - it.start;
        it.values_bytes = (it.w && n) ? n * it.w * 16 : 0;
        it.gran_words = (it.w && n) ? rect_granules((int)n, (int)it.w) : 0;
        it.ops = n + it.pj + 1;
    }
    const size_t budget = trace_budget("PA_SEARCH_TRACE_BUDGET_MB");  // (the re-filled columns dominate a chunk)
    std::vector<std::string> cigars(nq);
    std::vector<int64_t> starts(2 * nq);
    DeviceBuf d_values, d_vend, d_gran, d_ops, d_jobs, d_walk, d_wout, d_misc;
    if (!d_misc.alloc(16)) return PA_E_HIP;
    for (size_t c0 = 0; c0 < nq;) {
        size_t c1 = c0, bytes = 0;
        while (c1 < nq && (c1 == c0 || bytes + items[c1].values_bytes <= budget)) bytes += items[c1++].values_bytes;
        size_t vb = 0, vw = 0, gw = 0, ob = 0;
        std::vector<size_t> voff, vwoff, goff, ooff;
        for (size_t k = c0; k < c1; ++k) {
            voff.push_back(vb);
            vwoff.push_back(vw);
            goff.push_back(gw);
            ooff.push_back(ob);
            vb += items[k].values_bytes;
            vw += std::max<size_t>(items[k].w, 1);
            gw += items[k].gran_words;
            ob += items[k].ops;
        }
        // the left column of every window: v0 when it starts at column 0, V::one otherwise
        std::vector<uint64_t> vinit(2 * vw, 0);
        for (size_t k = c0; k < c1; ++k) {
            const TraceItem& it = items[k];
            uint64_t* dst = vinit.data() + 2 * vwoff[k - c0];
            if (it.start == 0) std::memcpy(dst, sb->v0.data() + 2 * sb->prof_word[sb->qp[it.q]], it.w * 16);
            else
                for (size_t j = 0; j < it.w; ++j) dst[2 * j] = ~0ull;
        }
        if (!d_values.alloc(std::max<size_t>(vb, 16)) || !upload(d_vend, vinit.data(), vinit.size() * 8, s) || !d_gran.alloc(std::max<size_t>(gw * 8, 16)) ||
            !hip_ok(hipMemsetAsync(d_gran.ptr, 0, std::max<size_t>(gw * 8, 16), s), "memset gran") || !d_ops.alloc(std::max<size_t>(ob, 16)))
            return PA_E_HIP;
        std::vector<StripJob> jobs;
        std::vector<WalkQuery> walk(c1 - c0);
        for (size_t k = c0; k < c1; ++k) {
            const TraceItem& it = items[k];
            const size_t p = sb->qp[it.q], n = it.end - it.start;
            const uint32_t* codes = sb->d_codes.as<uint32_t>() + sb->code_word[sb->qt[it.q]];
            const uint64_t* prof = sb->d_prof.as<uint64_t>() + 4 * sb->prof_word[p];
            uint64_t* vend = d_vend.as<uint64_t>() + 2 * vwoff[k - c0];
            uint64_t* values = reinterpret_cast<uint64_t*>(d_values.as<uint8_t>() + voff[k - c0]);
            if (it.w && n) {
                RectPlan r;
                r.a_codes = codes;
                r.col0 = (int)it.start;
                r.b_prof = reinterpret_cast<const uint32_t*>(prof);
                r.v = reinterpret_cast<uint32_t*>(vend);
                r.n = (int)n;
                r.w0 = 0;
                r.w1 = (int)it.w;
                r.hin_arr = sb->d_zero.as<uint8_t>();
                r.gran = d_gran.as<uint64_t>() + goff[k - c0];
                r.gran_stride = (n + 31) / 32;
                r.values = reinterpret_cast<uint32_t*>(values);
                r.fill_stride = (int)it.w;
                r.fill_word0 = 0;
                plan_rect(jobs, r);
            }
            WalkQuery& W = walk[k - c0];
            W.codes = codes;
            W.prof = prof;
            W.v0 = sb->d_v0.as<uint64_t>() + 2 * sb->prof_word[p];
            W.values = values;
            W.vend = vend;
            W.ops = d_ops.as<uint8_t>() + ooff[k - c0];
            W.w = (int32_t)it.w;
            W.start = (int32_t)it.start;
            W.pi = (int32_t)it.pi;
            W.pj = (int32_t)it.pj;
            W.target = it.target;
            W.cap = (int32_t)it.ops;
        }
        const int nw = (int)(c1 - c0);
        std::vector<WalkOut> wout(nw);
        std::vector<uint8_t> ops(ob);
        if (!upload(d_jobs, jobs.data(), jobs.size() * sizeof(StripJob), s) || !upload(d_walk, walk.data(), walk.size() * sizeof(WalkQuery), s) ||
            !d_wout.alloc(nw * sizeof(WalkOut)) || !hip_ok(hipMemsetAsync(d_misc.ptr, 0, 16, s), "memset misc") ||
            !launch_strips(d_jobs.as<StripJob>(), (int)jobs.size(), true, d_misc.as<uint32_t>(), s, true, /*scatter=*/true))
            return PA_E_HIP;
        hipLaunchKernelGGL(search_walk_kernel, dim3((nw + 63) / 64), dim3(64), 0, s, d_walk.as<WalkQuery>(), nw, d_wout.as<WalkOut>());
        if (!hip_ok(hipGetLastError(), "search_walk_kernel launch") ||
            !hip_ok(hipMemcpyAsync(wout.data(), d_wout.ptr, nw * sizeof(WalkOut), hipMemcpyDeviceToHost, s), "D2H") ||
            !hip_ok(hipMemcpyAsync(ops.data(), d_ops.ptr, ob, hipMemcpyDeviceToHost, s), "D2H") || !hip_ok(hipStreamSynchronize(s), "sync"))
            return PA_E_HIP;
        if (const int rc = check_device_error(d_misc, s)) return rc;
        for (size_t k = c0; k < c1; ++k) {
            const WalkOut& o = wout[k - c0];
            if (o.status != kWalkOk) {
                static const char* what[] = {"", "found a path cheaper than the target cost", "the first window does not reproduce the target cost",
                                             "bad trace, stuck", "trace ended inside the text with cost left", "path longer than its buffer"};
                return fail(PA_E_INTERNAL, "pa_search_batch_trace: query %u: %s", items[k].q, what[o.status < 6 ? o.status : 0]);
            }
            engine::Cigar cig;
            const uint8_t* op = ops.data() + ooff[k - c0];
            for (int32_t i = 0; i < o.nops; ++i) {
                const engine::CigarOp c = op[i] == '=' ? engine::CigarOp::Match
                                          : op[i] == 'X' ? engine::CigarOp::Sub
                                          : op[i] == 'D' ? engine::CigarOp::Del
                                                         : engine::CigarOp::Ins;
                cig.push_elem(engine::CigarElem{c, 1});
            }
            cig.reverse();
            cigars[items[k].q] = cig.to_string();
            starts[2 * items[k].q] = o.si;
            starts[2 * items[k].q + 1] = o.sj;
        }
        c0 = c1;
    }
    if (cigars_out)
        if (const int rc = give_cstrings(cigars, cigars_out)) return rc;
    if (start_out) std::memcpy(start_out, starts.data(), 2 * nq * sizeof(int64_t));
    return 0;
}

extern "C" void pa_search_batch_info(const pa_search_batch* sb, double* waves, double* packed, double* chained, double* lane_use) {
    const double w = sb ? (double)(sb->waves.size() + sb->jobs.size()) : 0;
    if (waves) *waves = w;
    if (packed) *packed = sb ? (double)(sb->nq - sb->chained.size()) : 0;
    if (chained) *chained = sb ? (double)sb->chained.size() : 0;
    if (lane_use) *lane_use = w > 0 ? sb->lanes_real / (64.0 * w) : 0;
}

extern "C" void pa_search_batch_destroy(pa_search_batch* sb) {
    if (!sb) return;
    (void)hipDeviceSynchronize();
    delete sb;
}
